"""utils.vector_quantization on the device (include/vtc_vq.h) against the
float64 numpy restatement of tests/vq_data.py and the fits stored in
tests/golden/vq.npz (tools/make_vq_golden.py).

Indices, counts, k, zero_index, iterations and converged are EQUAL to the
restatement.  Codebook, lengths and cost are within 1e-11 relative, the
lengths against max(1, |l|): the bound and the derivation of
tests/test_quantization_gpu.py.  A float64 sum of n terms in any order differs
by at most n * 2^-53 of the sum of magnitudes; the largest sums here run over
the 2 * VTC_VQ_ROWS + 3 = 4099 rows of the sparse fits, 4099 * 2^-53 =
4.6e-13; the device log2 is within a few ulp; the rest is margin.  (A block of
the step holds 2048 rows, well under the 10^4 at which 1e-11 would need
restating.)  The fixture keeps every assignment more than 1e-8 relative away
from a tie, so such a gap cannot flip one.  Where the codebook is an input the
device forms the same IEEE costs as numpy and the indices are equal whatever
the margin.  Every call is made twice and compared bitwise.  The largest gap
observed is printed (profiles/vq.txt records it).
"""
import ctypes

import numpy as np
import pytest
import torch

import helpers
import test_quantization_gpu as scalar_tests
import vq_data as data

pytestmark = pytest.mark.gpu

BOUND = 1e-11
DEVICE_STATE = ('codebook', 'lengths', 'counts', 'k', 'zero_index')
STATE = ('codebook', 'lengths', 'counts', 'cost', 'k', 'zero_index', 'active',
         'iterations')
same_bits, twice, gap_of, dev = (scalar_tests.same_bits, scalar_tests.twice,
                                 scalar_tests.gap_of, scalar_tests.dev)


def raw_assign(device, x_dev, book, k, lengths, lam, with_dequantized=True):
  """vtc_vq_assign itself: `book` (kmax, d) and `lengths` [kmax] or None as
  they are, k codewords in use.  Outputs start as 0xFF bytes."""
  import vtc_hip
  lib = vtc_hip.load_library()
  b, d = x_dev.shape
  book_dev = dev(book, device)
  lengths_dev = None if lengths is None else dev(lengths, device)
  k_dev = dev(np.array([k], np.int32), device)
  indices = torch.full((b,), -1, dtype=torch.int32, device=device)
  deq = torch.full((b, d), float('nan'), dtype=torch.float32, device=device)
  status = torch.full((1,), -1, dtype=torch.int64, device=device)
  vtc_hip.check(lib.vtc_vq_assign(
      vtc_hip.ptr(x_dev), b, d, vtc_hip.ptr(book_dev),
      vtc_hip.ptr(lengths_dev), vtc_hip.ptr(k_dev), book.shape[0], lam,
      vtc_hip.ptr(indices), vtc_hip.ptr(deq) if with_dequantized else None,
      vtc_hip.ptr(status), vtc_hip.current_stream(device)), 'vtc_vq_assign')
  return indices, deq, status


# ------------------------------------------------------------------- assign
def assign_shapes():
  for d in (1, 2, 23, 32):
    ks = [1, 2, 33, data.tile_codewords(d) + 1]   # one past a single LDS tile
    if d == 32:
      ks.append(data.MAX_CODEWORDS)
    for k in ks:
      for b in (1, 65, data.ASSIGN_ROWS + 3):
        yield b, d, k


@pytest.mark.parametrize('b,d,k', list(assign_shapes()))
def test_assign_and_dequantize(device, b, d, k):
  from utils import vector_quantization as vq
  x = data.vectors(1000 + 7 * b + 3 * d + k, b, d, scale=2.0)
  book = data.random_codebook(k + d, k, d)
  # at b = 65 the codebook has three slots more than are in use, never read
  kmax = min(k + 3, data.MAX_CODEWORDS) if b == 65 else k
  stored = np.full((kmax, d), np.nan)
  stored[:k] = book
  lengths = np.random.RandomState(k).uniform(1.0, 9.0, size=kmax)
  x_dev = dev(x, device)
  for lam, given in ((0.0, None), (0.0, np.full(kmax, np.inf)),
                     (0.05, lengths)):
    # the codebook is an input, so the device forms the same IEEE costs as
    # numpy: it takes an exact tie, not a small margin, to tell them apart
    want, margin, _ = data.assign(x, book, k, lengths, lam)
    assert margin > 0, margin
    indices, deq, status = twice(lambda: raw_assign(
        device, x_dev, stored, k, given, lam))
    assert np.array_equal(indices.cpu().numpy(), want), (b, d, k, lam)
    assert same_bits(deq.cpu().numpy(), data.dequantize(want, book))
    assert int(status) == 0
  # the Python entry points: pair, dictionary and array name the same quantiser
  want, _, _ = data.assign(x, book, k, lengths, 0.05)
  indices, deq = twice(lambda: vq.vector_assign(
      x_dev, (stored, np.array([k], np.int32)), lengths, 0.05,
      return_dequantized=True))
  assert indices.dtype == torch.int32 and deq.dtype == torch.float32
  assert np.array_equal(indices.cpu().numpy(), want)
  assert same_bits(deq.cpu().numpy(), data.dequantize(want, book))
  assert same_bits(twice(lambda: vq.vector_dequantize(indices, stored)), deq)
  counts = twice(lambda: vq.vector_index_counts(indices, kmax))
  assert counts.dtype == torch.int64
  assert np.array_equal(counts.cpu().numpy(), data.index_counts(want, kmax))
  nearest = twice(lambda: vq.vector_assign(x_dev, book))
  assert np.array_equal(nearest.cpu().numpy(), data.assign(x, book, k)[0])


def test_exact_ties_go_to_the_lowest_index(device):
  """Codewords and vectors on multiples of 0.5, the codewords in shuffled
  order: every cost is exact, so only the tie rule decides.  Then the same
  with lambda = 0.5 and whole-bit lengths, still exact.  -0.0 lands on the
  zero codeword."""
  rs = np.random.RandomState(9)
  d = 3
  grid = np.array([[a, c, e] for a in (-0.5, 0.0, 0.5) for c in (-0.5, 0.0, 0.5)
                   for e in (0.0, 1.0)])
  book = grid[rs.permutation(len(grid))]
  zero = int(np.nonzero((book == 0).all(1))[0][0])
  lengths = rs.randint(1, 4, size=len(book)).astype(np.float64)
  x = (rs.randint(-3, 4, size=(200, d)) * 0.25).astype(np.float32)
  x[0] = -0.0
  x[1] = 0.0
  x_dev = dev(x, device)
  for lam in (0.0, 0.5):
    want = np.zeros(len(x), np.int32)
    ties = 0
    for r in range(len(x)):
      costs = []
      for i in range(len(book)):
        dist = 0.0
        for t in range(d):
          e = float(x[r, t]) - book[i, t]
          dist = dist + e * e
        costs.append(dist + lam * lengths[i] if lam else dist)
      want[r] = costs.index(min(costs))          # the first of the minima
      ties += costs.count(min(costs)) > 1
    assert ties >= 50, ties
    assert np.array_equal(want, data.assign(x, book, len(book), lengths,
                                            lam)[0])
    got, deq, _ = twice(lambda: raw_assign(device, x_dev, book, len(book),
                                           lengths, lam))
    assert np.array_equal(got.cpu().numpy(), want), lam
    if lam == 0:
      assert want[0] == zero and want[1] == zero
      assert same_bits(deq.cpu().numpy()[:2], np.zeros((2, d), np.float32))


def test_nan_rows(device):
  """A row with any NaN component: index -1, a whole row of NaN, counted once
  in status however many of its components are NaN; infinities are numbers."""
  from utils import vector_quantization as vq
  import vtc_hip
  d = 23
  x = data.vectors(31, data.ASSIGN_ROWS + 3, d, scale=2.0)
  x[3, 5] = np.nan
  x[64, :] = np.nan
  x[255, 22] = np.nan
  x[256, 0] = np.nan
  x[7, 2] = np.inf
  book = data.random_codebook(32, 40, d)
  x_dev = dev(x, device)
  want, _, _ = data.assign(x, book, 40)
  assert (want < 0).sum() == 4 and want[7] == 0    # every distance inf: cell 0
  indices, deq, status = twice(lambda: raw_assign(device, x_dev, book, 40,
                                                  None, 0.0))
  assert np.array_equal(indices.cpu().numpy(), want)
  assert int(status) == 4
  got = deq.cpu().numpy()
  assert np.array_equal(np.isnan(got), np.repeat((want < 0)[:, None], d, 1))
  assert same_bits(got[want >= 0], data.dequantize(want, book)[want >= 0])
  counts = twice(lambda: vq.vector_index_counts(indices, 40)).cpu().numpy()
  assert counts.sum() == len(x) - 4
  with pytest.raises(ValueError, match='NaN'):
    vq.vector_lloyd(x_dev, book, max_iterations=2)
  with pytest.raises(NotImplementedError):
    vq.vector_assign(x_dev, np.zeros((4097, d)))
  with pytest.raises(NotImplementedError):
    vq.vector_assign(torch.zeros((4, 33), device=device), np.zeros((2, 33)))
  lib = vtc_hip.load_library()
  assert lib.vtc_vq_lloyd_step_workspace_bytes(5, 2, 4097) == 0


# --------------------------------------------------------------- Lloyd fits
GAPS = {}


def check_state(got, want, label):
  """Integers equal, floats within BOUND.  Returns the gaps."""
  for key in ('k', 'zero_index', 'counts'):
    assert np.array_equal(got[key], want[key]), (label, key)
  gaps = {'codebook': gap_of(got['codebook'], want['codebook']),
          'lengths': gap_of(got['lengths'], want['lengths'], floor=1.0),
          'cost': gap_of(got['cost'], want['cost'])}
  print('vq_gap %-16s codebook %.2e lengths %.2e cost %.2e'
        % (label, gaps['codebook'], gaps['lengths'], gaps['cost']))
  for key, gap in gaps.items():
    GAPS[key] = max(GAPS.get(key, 0.0), gap)
    assert gap <= BOUND, (label, key, gap)
  return gaps


def check_fit(result, want, label):
  assert result['iterations'] == int(want['iterations'][0]), label
  assert result['converged'] == bool(want['active'][0] == 0), label
  got = {key: result[key].cpu().numpy() for key in DEVICE_STATE}
  got['cost'] = result['cost']
  return check_state(got, want, label)


@pytest.mark.parametrize('name', sorted(data.FITS))
def test_vector_lloyd_matches_the_fixture(device, name):
  from utils import vector_quantization as vq
  g = helpers.load('vq')
  num_bins, lam, max_iterations, epsilon, pin_zero = data.FITS[name][3:]
  x, book = data.fit_inputs(name)
  x_dev = dev(x, device)
  start = twice(lambda: vq.initial_vector_codebook(x_dev, num_bins))
  assert start.dtype == torch.float64 and same_bits(start.cpu().numpy(), book)
  result = twice(lambda: vq.vector_lloyd(
      x_dev, start, lagrange_mult=lam, max_iterations=max_iterations,
      epsilon=epsilon, pin_zero=pin_zero))
  want = {key: g['%s_%s' % (name, key)] for key in
          data.STATE_FLOAT + data.STATE_INT}
  assert result['codebook'].dtype == torch.float64
  assert result['counts'].dtype == torch.int64
  assert result['k'].dtype == torch.int32
  assert result['codebook'].shape == book.shape
  check_fit(result, want, name)
  # the fitted quantiser, handed back as it is, assigns like the restatement
  indices = twice(lambda: vq.vector_assign(x_dev, result, lagrange_mult=lam))
  want_indices, margin, _ = data.assign(
      x, result['codebook'].cpu().numpy(), want['k'],
      result['lengths'].cpu().numpy(), lam)
  assert margin > data.MARGIN
  assert np.array_equal(indices.cpu().numpy(), want_indices)
  final, _, _ = data.assign(x, want['codebook'], want['k'], want['lengths'],
                            lam)
  assert np.array_equal(want_indices, final)
  if name in data.SPARSE:   # the seams: blocks of rows, tiles of codewords
    assert x.shape[0] == 2 * data.ROWS + 3
    assert book.shape[0] > data.tile_codewords(x.shape[1])
    z = int(want['zero_index'][0])
    if z >= 0:
      assert want['counts'][z] > x.shape[0] // 2


def raw_step(device, x_dev, state, lam, epsilon, pin_zero, in_place=False):
  """vtc_vq_lloyd_step itself from the numpy `state`: into a second state
  filled with 0xFF bytes, or in place.  Returns the state written, status
  and the input state read back."""
  import vtc_hip
  lib = vtc_hip.load_library()
  b, d = x_dev.shape
  kmax = state['codebook'].shape[0]
  before = {name: dev(state[name], device) for name in STATE}
  if in_place:
    after = before
  else:
    after = {name: torch.full_like(value, -1)
             for name, value in before.items()}
    for name in data.STATE_FLOAT:
      after[name].view(torch.int64).fill_(-1)      # 0xFF bytes: a NaN
  status = torch.full((1,), -1, dtype=torch.int64, device=device)
  ws_bytes = lib.vtc_vq_lloyd_step_workspace_bytes(b, d, kmax)
  ws = vtc_hip.workspace(ws_bytes, device)
  ws.fill_(255)
  struct = lambda t: vtc_hip.VqState(**{n: v.data_ptr()
                                        for n, v in t.items()})
  vtc_hip.check(lib.vtc_vq_lloyd_step(
      vtc_hip.ptr(x_dev), b, d, kmax, lam, epsilon, 1 if pin_zero else 0,
      ctypes.byref(struct(before)), ctypes.byref(struct(after)),
      vtc_hip.ptr(status), vtc_hip.ptr(ws), ws_bytes,
      vtc_hip.current_stream(device)), 'vtc_vq_lloyd_step')
  out = {name: value.cpu().numpy() for name, value in after.items()}
  out['status'] = status.cpu().numpy()
  if not in_place:
    for name in STATE:                             # the inputs were not written
      assert same_bits(before[name].cpu().numpy(),
                       np.ascontiguousarray(state[name])), name
  return out


@pytest.mark.parametrize('name', data.SPARSE)
def test_one_step_into_a_second_state_and_in_place(device, name):
  """The second step of every sparse fit (the first that makes the
  convergence test, and one that drops cells under lambda = 0.5): written into
  a separate state and in place, bit for bit the same, and the restatement's
  step."""
  lam, _, epsilon, pin_zero = data.FITS[name][4:]
  x, book = data.fit_inputs(name)
  x_dev = dev(x, device)
  state, _ = data.initial_state(x, book)
  state, _ = data.step(x, state, lam, epsilon, pin_zero)
  want, facts = data.step(x, state, lam, epsilon, pin_zero)
  assert facts['margin'] > data.MARGIN and facts['convergence'] is not None
  if lam:
    assert facts['lost'] > 0 and facts['moved'] > 0
  apart = twice(lambda: raw_step(device, x_dev, state, lam, epsilon, pin_zero))
  in_place = twice(lambda: raw_step(device, x_dev, state, lam, epsilon,
                                    pin_zero, in_place=True))
  for key in STATE + ('status',):
    assert same_bits(apart[key], in_place[key]), key
  assert apart['status'].tolist() == [0]
  for key in ('active', 'iterations'):
    assert np.array_equal(apart[key], want[key]), key
  check_state(apart, want, name + '_step2')
  knew = int(want['k'][0])
  assert (apart['codebook'][knew:] == 0).all()     # the slots past the new k
  assert (apart['lengths'][knew:] == 0).all()
  assert (apart['counts'][knew:] == 0).all()


def test_a_frozen_state_is_copied_bit_for_bit(device):
  """active == 0: all kmax slots of every array as they were, whatever they
  hold, and status 0 although a row is NaN; then a whole fit: the steps after
  convergence leave the state alone."""
  from utils import vector_quantization as vq
  rs = np.random.RandomState(12)
  b, d, kmax = 300, 23, 40
  x = data.vectors(12, b, d)
  x[5, 1] = np.nan
  state = {'codebook': rs.randn(kmax, d), 'lengths': rs.uniform(1, 9, kmax),
           'counts': rs.randint(0, 99, kmax).astype(np.int64),
           'cost': np.array([3.0, 2.0, 1.0]), 'k': np.array([33], np.int32),
           'zero_index': np.array([-1], np.int32),
           'active': np.zeros(1, np.int32),
           'iterations': np.array([7], np.int32)}
  got = twice(lambda: raw_step(device, dev(x, device), state, 0.5, 1e-3, True))
  for key in STATE:
    assert same_bits(got[key], np.ascontiguousarray(state[key])), key
  assert got['status'].tolist() == [0]
  name = 'sparse_ec'            # converges after 4 of its 6 steps
  lam, _, epsilon, pin_zero = data.FITS[name][4:]
  x, book = data.fit_inputs(name)
  short, longer = [twice(lambda: vq.vector_lloyd(
      dev(x, device), book, lagrange_mult=lam, max_iterations=n,
      epsilon=epsilon, pin_zero=pin_zero)) for n in (4, 9)]
  assert short['converged'] and short['iterations'] == 4
  scalar_tests.assert_same(short, longer)


def test_every_row_nan_in_one_step(device):
  """The quantiser is copied as it was, cost = NaN, active = 0, iterations + 1,
  status = b."""
  b, d, kmax = 70, 5, 6
  x = np.full((b, d), np.nan, np.float32)
  x[:, 1::2] = 1.0                                 # some components are numbers
  book = data.random_codebook(5, kmax, d)
  state = {'codebook': book, 'lengths': np.arange(1.0, kmax + 1),
           'counts': np.arange(kmax, dtype=np.int64), 'cost': np.full(3, 1e9),
           'k': np.array([4], np.int32), 'zero_index': np.array([0], np.int32),
           'active': np.ones(1, np.int32),
           'iterations': np.array([2], np.int32)}
  want, _ = data.step(x, state, 0.5, 1e-3, True)
  assert np.isnan(want['cost']).all() and want['active'][0] == 0
  got = twice(lambda: raw_step(device, dev(x, device), state, 0.5, 1e-3, True))
  for key in DEVICE_STATE:
    assert same_bits(got[key], np.ascontiguousarray(state[key])), key
  assert np.isnan(got['cost']).all()
  assert got['active'].tolist() == [0] and got['iterations'].tolist() == [3]
  assert got['status'].tolist() == [b]


def test_pinned_zero_without_members_keeps_its_slot(device):
  """No row is nearest to the zero vector: pinned, its codeword stays with no
  member and length +inf; unpinned it is removed and zero_index becomes -1."""
  from utils import vector_quantization as vq
  rs = np.random.RandomState(8)
  x = (rs.choice([-1.0, 1.0], size=(65, 2)) *
       rs.uniform(0.8, 1.6, size=(65, 2))).astype(np.float32)
  book = np.array([[-1.0, -1.0], [0.0, 0.0], [1.0, 1.0], [-1.0, 1.0],
                   [1.0, -1.0]])
  for pin_zero in (True, False):
    result = twice(lambda: vq.vector_lloyd(
        dev(x, device), book, max_iterations=3, epsilon=1e-3,
        pin_zero=pin_zero))
    want, history, margin = data.fit(x, book, 0.0, 3, 1e-3, pin_zero)
    assert min([margin] + [f['margin'] for f in history]) > data.MARGIN
    check_fit(result, want, 'pinned' if pin_zero else 'removed')
    got = {key: result[key].cpu().numpy() for key in DEVICE_STATE}
    if pin_zero:
      assert got['k'][0] == 5 and got['zero_index'][0] == 1
      assert (got['codebook'][1] == 0.0).all()
      assert np.isposinf(got['lengths'][1]) and got['counts'][1] == 0
    else:
      assert got['k'][0] == 4 and got['zero_index'][0] == -1
      assert (got['codebook'][4] == 0.0).all()


def test_the_largest_quantiser_in_one_step(device):
  """kmax = 4096 with d = 32, the largest state the header allows: most cells
  have no member and are dropped, the kept ones move down thousands of slots.
  (Two blocks of rows are crossed by the sparse fits; the rows here are few so
  that the restatement stays quick.)"""
  b, d, kmax = 2 * data.ASSIGN_ROWS + 3, 32, data.MAX_CODEWORDS
  x = data.vectors(41, b, d)
  rs = np.random.RandomState(43)
  state = {'codebook': data.random_codebook(42, kmax, d, scale=0.7),
           'lengths': rs.uniform(1.0, 12.0, kmax),
           'counts': np.zeros(kmax, np.int64),
           'cost': np.array([1e9, 0.0, 0.0]), 'k': np.array([kmax], np.int32),
           'zero_index': np.array([0], np.int32),
           'active': np.ones(1, np.int32),
           'iterations': np.array([1], np.int32)}
  want, facts = data.step(x, state, 0.5, 1e-3, True)
  assert facts['margin'] > data.MARGIN and facts['lost'] > 3000
  assert facts['moved'] > 0 and want['active'][0] == 1
  got = twice(lambda: raw_step(device, dev(x, device), state, 0.5, 1e-3, True,
                               in_place=True))
  for key in ('active', 'iterations'):
    assert np.array_equal(got[key], want[key]), key
  check_state(got, want, 'largest')


# ---------------------------------------------------------- rate-distortion
@pytest.fixture(scope='module')
def scene(device):
  s = data.scene()
  on = {key: dev(s[key], device)
        for key in ('patches', 'dictionary', 'codes', 'image')}
  on['positions'] = s['positions']
  on['host'] = s
  return on


def expected_distortion(device, scene, dequantized, full):
  """compute_RD_point's distortion of the restatement's dequantised codes."""
  from utils import quantization
  back = quantization._reconstruct(dev(dequantized, device),
                                   scene['dictionary'])
  params = {'patch_dim': (data.PATCH, data.PATCH),
            'patch_positions': scene['positions']}
  return quantization._distortion(scene['patches'], back,
                                  params if full else None)


@pytest.mark.parametrize('name', sorted(data.POINTS))
def test_experiment_entry_points(device, scene, name):
  """Mod2 / Mod3_compute_RD_point as the experiment calls them: the training
  call, then the test call with what it returned and the images' positions.
  Rate against the restatement's within 1e-12 relative, the bound of
  test_compute_RD_point of tests/test_quantization_gpu.py; the distortions
  equal to compute_pSNR and compute_ssim of the patches rebuilt from the
  restatement's dequantised codes, as there."""
  from utils import image_processing
  from utils import vector_quantization as quantization
  g = helpers.load('vq')
  variant, scal_mult, vec_mult = data.POINTS[name]
  entry = (quantization.Mod2_compute_RD_point if variant == 2
           else quantization.Mod3_compute_RD_point)
  codes, patches, dictionary = (scene['codes'], scene['patches'],
                                scene['dictionary'])
  widths = [data.SCAL_WIDTH] * len(data.SCAL_CLUSTS)
  params = {'patch_dim': (data.PATCH, data.PATCH),
            'patch_positions': scene['positions']}
  assert torch.equal(image_processing.assemble_image_from_patches(
      patches, (data.PATCH, data.PATCH), scene['positions'])[:, :, 0],
                     scene['image'])

  def train(vec_multiplier):
    return entry(codes, patches, dictionary, data.SCAL_CLUSTS, data.VEC_CLUST,
                 scal_quant_multiplier=scal_mult, scal_binwidths=widths,
                 vec_quant_multiplier=vec_multiplier,
                 vec_init_num_bins=100000, max_iterations=data.RD_ITERATIONS,
                 epsilon=data.RD_EPSILON)
  out = twice(lambda: train(vec_mult))
  assert len(out) == 8 and out[5:] == (None, None, None)
  rate, dist, scal_cbook, vec_cbook, vec_cw_len = out[:5]
  assert vec_cw_len is vec_cbook['lengths'] and set(dist) == {'pSNR'}
  if variant == 3:
    assert scal_cbook['lagrange_mult'] == scal_mult

  want = data.rd_point(name, scene['host'])
  assert want['margin'] > data.MARGIN
  assert abs(want['rate'] - float(g[name + '_rate'])) <= 1e-12 * want['rate']
  got_vec = {key: vec_cbook[key].cpu().numpy() for key in DEVICE_STATE}
  got_vec['cost'] = want['vec']['cost']            # a host value of the fit
  check_state(got_vec, want['vec'], name + '_vec')
  print('vq_rd %s rate %.9f restatement %.9f pSNR %.6f restatement %.6f'
        % (name, rate, want['rate'], dist['pSNR'], want['psnr_patches']))
  assert abs(rate - want['rate']) <= 1e-12 * want['rate']
  assert dist == expected_distortion(device, scene, want['dequantized'], False)
  assert abs(dist['pSNR'] - want['psnr_patches']) <= 1e-4
  assert 10.0 < dist['pSNR'] < 80.0

  test_rate, test_dist = twice(lambda: entry(
      codes, patches, dictionary, data.SCAL_CLUSTS, data.VEC_CLUST,
      vec_quant_multiplier=vec_mult, precomputed_scal_codebook=scal_cbook,
      precomputed_vec_codebook=vec_cbook,
      precomputed_vec_codebook_lengths=vec_cw_len,
      precomputed_huff_tab1=out[5], precomputed_huff_tab2=out[6],
      precomputed_huff_tab3=out[7], fullimg_reshape_params=params))
  assert test_rate == rate
  assert set(test_dist) == {'pSNR', 'SSIM', 'pSNR_patches'}
  assert test_dist == expected_distortion(device, scene, want['dequantized'],
                                          True)
  assert test_dist['pSNR_patches'] == dist['pSNR']
  assert 0.0 < test_dist['SSIM'] < 1.0

  # a larger multiplier of the vector part must not raise the rate
  assert train(4 * vec_mult)[0] <= rate


def test_mixed_point_refuses_bad_clusters(device, scene):
  from utils import vector_quantization as vq
  codes, patches, dictionary = (scene['codes'], scene['patches'],
                                scene['dictionary'])
  scal = (np.zeros((2, 1)), np.ones(2, np.int32))
  book = np.zeros((1, 2))
  for scal_clusts, vec_clust in (([0, 1], [1, 2]), ([0, 0], [2, 3]),
                                 ([0, 1], [2, 64]), ([-1, 1], [2, 3])):
    with pytest.raises(ValueError):
      vq.compute_RD_point_mixed(codes, patches, dictionary, scal_clusts, scal,
                                vec_clust, book)
  # coefficients in neither cluster are zero and cost no bits
  rate, dist = twice(lambda: vq.compute_RD_point_mixed(
      codes, patches, dictionary, [0, 1], scal, [2, 3], book))
  assert rate == 0.0
  assert dist == expected_distortion(
      device, scene, np.zeros(codes.shape, np.float32), False)


def test_report_the_largest_gaps():
  print('vq_largest_gap codebook %.2e lengths %.2e cost %.2e (bound %.0e)'
        % (GAPS.get('codebook', 0.0), GAPS.get('lengths', 0.0),
           GAPS.get('cost', 0.0), BOUND))
