"""utils.quantization on the device (include/vtc_quant.h) against the float64
numpy restatement of tests/quantization_data.py and the fits stored in
tests/golden/quantization.npz (tools/make_quantization_golden.py).

Indices, counts, k, zero_index, iterations and converged are EQUAL to the
restatement.  Codebooks, lengths and cost are within 1e-11 relative, the
lengths against max(1, |l|): a float64 sum of at most VTC_QUANT_ROWS + 3 = 515
terms in any order differs by at most 515 * 2^-53 = 5.7e-14 of the sum of
magnitudes, the device log2 is within a few ulp (OpenCL's conformance bound is
3), the rest is margin -- the bound and the derivation of
tests/test_code_stats_gpu.py.  The fixture keeps every assignment more than
1e-8 relative away from a tie, so such a gap cannot flip one.  Every call is
made twice and compared bitwise.  The largest gap observed is printed
(profiles/quantization.txt records it).
"""
import numpy as np
import pytest
import torch

import helpers
import quantization_data as data

pytestmark = pytest.mark.gpu

BOUND = 1e-11
DEVICE_STATE = ('codebooks', 'lengths', 'counts', 'k', 'zero_index')


def same_bits(a, b):
  """Equality of bit patterns: NaN and -0.0 are what they are."""
  if torch.is_tensor(a):
    a, b = a.cpu().numpy(), b.cpu().numpy()
  a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
  if a.dtype == bool:
    return a.shape == b.shape and np.array_equal(a, b)
  return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(
      a.view(np.uint8), b.view(np.uint8))


def assert_same(a, c, label='result'):
  """Two results of the same call: tensors and arrays have the same bits,
  containers the same members, everything else is equal."""
  if torch.is_tensor(a) or isinstance(a, np.ndarray):
    assert type(a) is type(c) and same_bits(a, c), (
        '%s differs between two calls' % (label,))
  elif isinstance(a, dict):
    assert isinstance(c, dict) and list(a) == list(c), label
    for key in a:
      assert_same(a[key], c[key], '%s[%r]' % (label, key))
  elif isinstance(a, (tuple, list)):
    assert type(a) is type(c) and len(a) == len(c), label
    for n, (x, y) in enumerate(zip(a, c)):
      assert_same(x, y, '%s[%d]' % (label, n))
  else:
    assert a == c or (a != a and c != c), (
        '%s differs between two calls' % (label,))


def twice(fn):
  """fn() called twice and the two results compared bitwise.  Returns the
  first."""
  first, second = fn(), fn()
  assert_same(first, second)
  return first


def gap_of(got, want, floor=0.0):
  """Largest |got - want| / max(floor, |want|) over the finite entries; the
  infinite ones must sit in the same places."""
  assert got.shape == want.shape
  assert np.array_equal(np.isinf(got), np.isinf(want))
  assert not np.isnan(got).any() and not np.isnan(want).any()
  ok = np.isfinite(want)
  scale = np.maximum(np.abs(want[ok]), floor)
  diff = np.abs(got[ok] - want[ok])
  assert (diff[scale == 0] == 0).all()
  return float((diff[scale > 0] / scale[scale > 0]).max(initial=0.0))


def dev(array, device):
  return torch.from_numpy(np.ascontiguousarray(array)).to(device)


# ------------------------------------------------------------------- assign
@pytest.mark.parametrize('k', (1, 2, 33, 1024))
@pytest.mark.parametrize('s', (1, 3, 67))
@pytest.mark.parametrize('b', (1, 65, data.ROWS + 3))
def test_assign_counts_and_dequantize(device, b, s, k):
  from utils import quantization
  x = data.codes(100 + b + s + k, b, s)
  books, kk = data.grid_codebooks(s, k, {1: 1.0, 2: 1.0, 33: 0.375,
                                          1024: 1.0 / 64}[k])
  kk = kk.copy()
  kk[::2] = np.maximum(1, kk[::2] - kk[::2] // 3)   # columns use fewer cells
  books = np.where(np.arange(k)[None, :] < kk[:, None], books, np.inf)
  lengths = np.random.RandomState(k).uniform(1.0, 9.0, size=(s, k))
  x_dev = dev(x, device)
  for lam in (0.0, 0.05):
    # the codebooks are inputs, so the device forms the same IEEE costs as
    # numpy: it takes an exact tie, not a small margin, to tell them apart
    want, margin = data.assign(x, books, kk, lengths, lam)
    assert margin > 0, margin
    indices, deq = twice(lambda: quantization.assign(
        x_dev, (books, kk), lengths if lam else None, lam,
        return_dequantized=True))
    assert indices.dtype == torch.int32 and deq.dtype == torch.float32
    assert np.array_equal(indices.cpu().numpy(), want), (b, s, k, lam)
    assert same_bits(deq.cpu().numpy(), data.dequantize(want, books))
    assert same_bits(twice(lambda: quantization.dequantize_assignments(
        indices, (books, kk))), deq)
    counts = twice(lambda: quantization.index_counts(indices, k))
    assert counts.dtype == torch.int64
    assert np.array_equal(counts.cpu().numpy(), data.index_counts(want, k))
  # the padded array alone names the same quantiser
  assert torch.equal(twice(lambda: quantization.assign(x_dev, books)), dev(
      data.assign(x, books, kk)[0], device))


def test_exact_ties_go_to_the_lowest_index(device):
  """Codewords at multiples of 0.5 in no particular order, codes on the
  midpoints: every cost is exact, so only the tie rule decides.  Then the same
  with lambda = 0.5 and whole-bit lengths, still exact."""
  from utils import quantization
  books = np.array([[1.0, -0.5, 0.0, 0.5, -1.0, 1.5],
                    [0.5, 0.0, -0.5, -1.0, 1.0, np.inf]])
  k = np.array([6, 5], np.int32)
  lengths = np.array([[1.0, 2.0, 1.0, 3.0, 2.0, 1.0],
                      [2.0, 1.0, 2.0, 1.0, 3.0, np.inf]])
  x = np.array([[0.25, 0.25], [-0.75, -0.75], [0.75, 0.75], [-0.25, -0.25],
                [1.25, 1.25], [0.0, -0.0], [0.5, -0.5], [-1.0, 2.0],
                [1.75, -3.0]], np.float32)
  for lam in (0.0, 0.5):
    want = np.zeros(x.shape, np.int32)
    ties = 0
    for r in range(x.shape[0]):
      for j in range(2):
        costs = [(float(x[r, j]) - books[j, i]) ** 2 +
                 (lam * lengths[j, i] if lam else 0.0) for i in range(k[j])]
        want[r, j] = costs.index(min(costs))   # the first of the minima
        ties += costs.count(min(costs)) > 1
    assert ties >= 6
    got = twice(lambda: (quantization.assign(dev(x, device), (books, k),
                                             lengths, lam),))[0]
    assert np.array_equal(got.cpu().numpy(), want), lam


def test_nan_codes_and_negative_zero(device):
  from utils import quantization
  import vtc_hip
  books = np.array([[-1.0, 0.0, 1.0], [0.5, -0.5, 0.0]])
  k = np.array([3, 3], np.int32)
  x = np.array([[np.nan, -0.0], [-0.0, np.nan], [0.9, np.nan], [np.inf, 0.0],
                [-np.inf, 0.4]], np.float32)
  x_dev = dev(x, device)
  indices, deq, status = twice(lambda: quantization._assign(
      x_dev, (books, k), None, 0.0, True))
  want = np.array([[-1, 2], [1, -1], [2, -1], [0, 2], [0, 0]], np.int32)
  assert np.array_equal(indices.cpu().numpy(), want)
  assert np.array_equal(want, data.assign(x, books, k)[0])
  assert int(status) == 3
  got = deq.cpu().numpy()
  assert np.array_equal(np.isnan(got), want < 0)
  assert same_bits(got[want >= 0], data.dequantize(want, books)[want >= 0])
  counts = twice(lambda: quantization.index_counts(indices, 3)).cpu().numpy()
  assert counts.tolist() == [[2, 1, 1], [1, 0, 2]]
  with pytest.raises(ValueError, match='NaN'):
    quantization.scalar_lloyd(x_dev, (books, k), max_iterations=2)
  with pytest.raises(NotImplementedError):
    quantization.assign(x_dev, np.zeros((2, 1025)))
  lib = vtc_hip.load_library()
  assert lib.vtc_quant_lloyd_step_workspace_bytes(5, 2, 1025) == 0


# --------------------------------------------------------------- Lloyd fits
def check_fit(result, want, label):
  gaps = {}
  for key in ('k', 'zero_index', 'counts'):
    assert np.array_equal(result[key].cpu().numpy(), want[key]), (label, key)
  assert np.array_equal(result['iterations'], want['iterations']), label
  assert np.array_equal(result['converged'], want['active'] == 0), label
  gaps['codebooks'] = gap_of(result['codebooks'].cpu().numpy(),
                             want['codebooks'])
  gaps['lengths'] = gap_of(result['lengths'].cpu().numpy(), want['lengths'],
                           floor=1.0)
  gaps['cost'] = gap_of(result['cost'], want['cost'])
  print('quantization_gap %-10s codebooks %.2e lengths %.2e cost %.2e'
        % (label, gaps['codebooks'], gaps['lengths'], gaps['cost']))
  for key, gap in gaps.items():
    assert gap <= BOUND, (label, key, gap)
  return gaps


@pytest.mark.parametrize('name', sorted(data.FITS))
def test_scalar_lloyd_matches_the_fixture(device, name):
  from utils import quantization
  g = helpers.load('quantization')
  lam, max_iterations, epsilon, pin_zero = data.FITS[name][5:]
  x, books, k = data.fit_inputs(name)
  x_dev = dev(x, device)
  result = twice(lambda: quantization.scalar_lloyd(
      x_dev, (books, k), lagrange_mult=lam, max_iterations=max_iterations,
      epsilon=epsilon, pin_zero=pin_zero))
  want = {key: g['%s_%s' % (name, key)] for key in
          data.STATE_FLOAT + data.STATE_INT}
  assert result['codebooks'].dtype == torch.float64
  assert result['counts'].dtype == torch.int64
  assert result['k'].dtype == torch.int32
  check_fit(result, want, name)
  # the fitted quantiser, handed back as it is, assigns like the restatement
  indices = twice(lambda: quantization.assign(x_dev, result,
                                              lagrange_mult=lam))
  fitted = result['codebooks'].cpu().numpy()
  want_indices, margin = data.assign(x, fitted, want['k'],
                                     result['lengths'].cpu().numpy(), lam)
  assert margin > data.MARGIN
  assert np.array_equal(indices.cpu().numpy(), want_indices)


def test_pinned_zero_without_members_keeps_its_slot(device):
  """No code is nearest to 0.0: the pinned codeword stays, with no member and
  length +inf, and lambda == 0 never evaluates that length.  Unpinned, it is
  removed and zero_index becomes -1."""
  from utils import quantization
  rs = np.random.RandomState(8)
  x = (rs.choice([-1.0, 1.0], size=(65, 3)) *
       rs.uniform(0.8, 1.6, size=(65, 3))).astype(np.float32)
  books, k = data.grid_codebooks(3, 3, 1.0)   # -1, 0, 1
  for pin_zero in (True, False):
    result = twice(lambda: quantization.scalar_lloyd(
        dev(x, device), (books, k), max_iterations=3, epsilon=1e-3,
        pin_zero=pin_zero))
    want, history, margin = data.fit(x, books, k, 0.0, 3, 1e-3, pin_zero)
    assert margin > data.MARGIN
    check_fit(result, want, 'pinned' if pin_zero else 'removed')
    got = {key: result[key].cpu().numpy() for key in DEVICE_STATE}
    if pin_zero:
      assert (got['k'] == 3).all() and (got['zero_index'] == 1).all()
      assert (got['codebooks'][:, 1] == 0.0).all()
      assert np.isposinf(got['lengths'][:, 1]).all()
      assert (got['counts'][:, 1] == 0).all()
    else:
      assert (got['k'] == 2).all() and (got['zero_index'] == -1).all()
      assert (got['codebooks'][:, 2] == 0.0).all()


def test_a_frozen_column_is_left_alone_by_later_steps(device):
  """Columns that have converged after 6 steps are bit for bit the same after
  9: codebooks, lengths, counts, cost, k, zero_index and iterations."""
  from utils import quantization
  name = 'grid33_ec'
  lam, _, epsilon, pin_zero = data.FITS[name][5:]
  x, books, k = data.fit_inputs(name)
  x_dev = dev(x, device)
  short, longer = [twice(lambda: quantization.scalar_lloyd(
      x_dev, (books, k), lagrange_mult=lam, max_iterations=n, epsilon=epsilon,
      pin_zero=pin_zero)) for n in (6, 9)]
  frozen = short['converged']
  assert frozen.any() and not frozen.all()
  assert longer['converged'][frozen].all()
  assert (longer['iterations'][~frozen] > 6).all()
  for key in DEVICE_STATE:
    assert same_bits(short[key].cpu().numpy()[frozen],
                     longer[key].cpu().numpy()[frozen]), key
  for key in ('cost', 'iterations'):
    assert same_bits(short[key][frozen], longer[key][frozen]), key


# kmax -> columns of one workgroup's tile (QuantTile of csrc/quantization.hip):
# 32 halved until the LDS fits 64 KiB.  Plain assign, lambda == 0 / != 0, and
# a step with lambda != 0:
#   100: 32 / 32 / 16     300: 16 / 8 / 8     600: 8 / 4 / 4     959: 8 / 4 / 2
# 959 is the largest kmax whose 4-column tile of a plain assign with lengths
# fits: 4 * 959 * 16 + 128 = 61504 bytes.  35 columns: more than one tile of
# every width, and a last tile that is not full.
@pytest.mark.parametrize('kmax', (100, 300, 600, 959))
def test_every_tile_width(device, kmax):
  from utils import quantization
  b, s, lam = data.ROWS + 3, 35, 0.05
  x = data.codes(7000 + kmax, b, s)
  books, k = data.grid_codebooks(s, kmax, 16.0 / kmax)
  k = k.copy()
  k[1::3] -= kmax // 5                       # columns that use fewer cells
  x_dev = dev(x, device)
  lengths = np.random.RandomState(kmax).uniform(1.0, 9.0, size=(s, kmax))
  for lam_assign in (0.0, lam):
    want, margin = data.assign(x, books, k, lengths, lam_assign)
    assert margin > 0, margin                # the codebooks are inputs
    indices, deq = twice(lambda: quantization.assign(
        x_dev, (books, k), lengths if lam_assign else None, lam_assign,
        return_dequantized=True))
    assert np.array_equal(indices.cpu().numpy(), want), (kmax, lam_assign)
    assert same_bits(deq.cpu().numpy(), data.dequantize(want, books))
  for lam_fit in (0.0, lam):
    result = twice(lambda: quantization.scalar_lloyd(
        x_dev, (books, k), lagrange_mult=lam_fit, max_iterations=2,
        epsilon=1e-3))
    want, history, margin = data.fit(x, books, k, lam_fit, 2, 1e-3, True)
    assert min([margin] + [f['margin'] for f in history]) > data.MARGIN
    assert (want['k'] < k).any()             # columns were compacted
    check_fit(result, want, 'kmax%d_%g' % (kmax, lam_fit))


def test_a_column_of_nan_codes_in_one_step(device):
  """vtc_quant_lloyd_step itself, into a second state filled with 0xFF: an
  active column whose codes are all NaN keeps its quantiser bit for bit, gets
  cost NaN, active 0 and iterations + 1; status[0] counts the NaN codes of
  the active columns and not those of a frozen one."""
  import ctypes
  import vtc_hip
  lib = vtc_hip.load_library()
  b, s, kmax, lam = 65, 4, 5, 0.05
  x = data.codes(65, b, s, zeros=0.3)
  x[:, 1] = np.nan                           # active, nothing to fit
  x[[3, 40], 0] = np.nan                     # active, two codes missing
  x[7, 2] = np.nan                           # frozen: not read
  books, _ = data.grid_codebooks(s, kmax, 1.0)
  k = np.array([5, 4, 5, 3], np.int32)
  state = {
      'codebooks': np.where(np.arange(kmax)[None, :] < k[:, None], books, 7.0),
      'lengths': np.random.RandomState(5).uniform(1.0, 4.0, size=(s, kmax)),
      'counts': np.arange(s * kmax, dtype=np.int64).reshape(s, kmax),
      'cost': np.full((s, 3), 1e9), 'k': k,
      'zero_index': data.zero_points(books, k),
      'active': np.array([1, 1, 0, 1], np.int32),
      'iterations': np.array([0, 4, 2, 1], np.int32)}
  want, facts = data.step(x, state, lam, 1e-3, True)
  assert facts['margin'] > data.MARGIN
  assert np.isnan(want['cost'][1]).all() and want['active'][1] == 0
  assert want['iterations'].tolist() == [1, 5, 2, 2]

  x_dev = dev(x, device)
  before = {name: dev(value, device) for name, value in state.items()}
  ws_bytes = lib.vtc_quant_lloyd_step_workspace_bytes(b, s, kmax)
  ws = vtc_hip.workspace(ws_bytes, device)

  def step():
    after = {name: torch.full_like(value, -1) for name, value in before.items()}
    for name in data.STATE_FLOAT:
      after[name].view(torch.int64).fill_(-1)      # 0xFF bytes: a NaN
    status = torch.full((1,), -1, dtype=torch.int64, device=device)
    struct = lambda d: vtc_hip.QuantState(**{n: v.data_ptr()
                                             for n, v in d.items()})
    vtc_hip.check(lib.vtc_quant_lloyd_step(
        vtc_hip.ptr(x_dev), b, s, kmax, lam, 1e-3, 1,
        ctypes.byref(struct(before)), ctypes.byref(struct(after)),
        vtc_hip.ptr(status), vtc_hip.ptr(ws), ws.numel(),
        vtc_hip.current_stream(device)), 'vtc_quant_lloyd_step')
    after['status'] = status
    return {name: value.cpu().numpy() for name, value in after.items()}

  got = twice(step)
  for name, value in state.items():            # the inputs were not written
    assert same_bits(before[name].cpu().numpy(), value), name
  assert got['status'].tolist() == [b + 2]
  for name in data.STATE_INT:
    assert np.array_equal(got[name], want[name]), name
  for name in ('codebooks', 'lengths', 'counts', 'k', 'zero_index'):
    assert same_bits(got[name][1], state[name][1]), name   # all kmax slots
    assert same_bits(got[name][2], state[name][2]), name
  assert np.isnan(got['cost'][1]).all()
  assert same_bits(got['cost'][2], state['cost'][2])
  live = [0, 3]
  assert gap_of(got['codebooks'][live], want['codebooks'][live]) <= BOUND
  assert gap_of(got['lengths'][live], want['lengths'][live], 1.0) <= BOUND
  assert gap_of(got['cost'][live], want['cost'][live]) <= BOUND


# ---------------------------------------------------------- rate-distortion
@pytest.fixture(scope='module')
def scene(device):
  """8 x 8 patches of a 40 x 48 synthetic image, a 128-atom random dictionary
  and the codes of the FISTA plugin."""
  from analysis_transforms.fully_connected import ista_fista
  from utils import image_processing
  rs = np.random.RandomState(40)
  v, u = np.mgrid[0:40, 0:48]
  image = (60 * np.sin(v / 5.0) * np.cos(u / 7.0) + 0.5 * v - 0.3 * u +
           4 * rs.randn(40, 48)).astype(np.float32)
  image_dev = dev(image, device)
  patches, positions = image_processing.patches_from_single_image(
      image_dev[:, :, None], (8, 8), flatten_patches=True)
  dictionary = dev(helpers.unit_rows(41, 128, 64), device)
  codes = ista_fista.run(patches, dictionary, 2.0, 60)
  torch.cuda.synchronize(device)
  assert patches.shape == (30, 64) and codes.shape == (30, 128)
  share = float((codes == 0).float().mean())
  assert 0.2 < share < 0.995, share
  return {'patches': patches.contiguous(), 'positions': positions,
          'dictionary': dictionary, 'codes': codes.contiguous(),
          'image': image_dev}


def huffman_on_indices_bits(counts):
  """Bits of a Huffman code of each column's indices, trained on them."""
  from utils import jpeg
  total = 0
  for column in counts:
    seen = {i: int(n) for i, n in enumerate(column) if n}
    if len(seen) == 1:
      total += sum(seen.values())   # one symbol still costs a bit each
      continue
    table = jpeg.compute_huffman_table(seen)
    total += sum(n * len(table[i]) for i, n in seen.items())
  return total


@pytest.mark.parametrize('source_code', ('jpeg', 'entropy'))
def test_compute_RD_point(device, scene, source_code):
  from utils import image_processing
  from utils import jpeg
  from utils import plotting
  from utils import quantization
  codes, patches, dictionary = (scene['codes'], scene['patches'],
                                scene['dictionary'])
  summary = plotting.code_summary(codes)
  books, k = quantization.uniform_codebooks(
      summary['min'].cpu().numpy(), summary['max'].cpu().numpy(), 4.0)
  zero = quantization.cbook_inds_of_zero_pts((books, k))
  assert (zero >= 0).all() and k.max() > 2
  params = {'patch_dim': (8, 8), 'patch_positions': scene['positions']}

  def point(full):
    rate, distortion, tables = quantization.compute_RD_point(
        codes, patches, dictionary, (books, k), source_code=source_code,
        fullimg_reshape_params=params if full else None)
    return rate, distortion, tables
  rate, distortion, tables = twice(lambda: point(True))

  x = codes.cpu().numpy()
  want_indices, margin = data.assign(x, books, k)
  assert margin > data.MARGIN
  indices, deq = twice(lambda: quantization.assign(
      codes, (books, k), return_dequantized=True))
  assert np.array_equal(indices.cpu().numpy(), want_indices)
  counts = data.index_counts(want_indices, books.shape[1])
  with np.errstate(divide='ignore', invalid='ignore'):
    terms = np.where(counts > 0, -counts * np.log2(counts / 30.0), 0.0)
  entropy_rate = terms.sum() / patches.numel()
  if source_code == 'jpeg':
    levels = dev((want_indices - zero[None, :]).astype(np.int32), device)
    assert tables == jpeg.tables_from_counts(*jpeg.symbol_counts(levels))
    bits = jpeg.stream_bits(levels, tables[0], tables[1])
    assert rate == int(bits.to(torch.int64).sum()) / float(patches.numel())
    # the tables are reused when given
    again = twice(lambda: quantization.compute_RD_point(
        codes, patches, dictionary, (books, k), tables=tables))
    assert again[0] == rate and again[2] is tables
  else:
    assert tables is None
    assert abs(rate - entropy_rate) <= 1e-12 * entropy_rate
  assert entropy_rate <= (huffman_on_indices_bits(counts) /
                          float(patches.numel()))

  reconstruction = twice(lambda: quantization._reconstruct(deq, dictionary))
  want = data.dequantize(want_indices, books).astype(np.float64) @ (
      dictionary.cpu().numpy().astype(np.float64))
  assert np.abs(reconstruction.cpu().numpy() - want).max() <= (
      1e-5 * np.abs(want).max())
  original = image_processing.assemble_image_from_patches(
      patches, (8, 8), scene['positions'])[:, :, 0].contiguous()
  assert torch.equal(original, scene['image'])
  rebuilt = image_processing.assemble_image_from_patches(
      reconstruction, (8, 8), scene['positions'])[:, :, 0].contiguous()
  assert distortion == {
      'pSNR_patches': plotting.compute_pSNR(patches, reconstruction),
      'pSNR': plotting.compute_pSNR(original, rebuilt),
      'SSIM': plotting.compute_ssim(original, rebuilt)}
  assert 10.0 < distortion['pSNR'] < 80.0 and 0.0 < distortion['SSIM'] < 1.0
  _, patch_only, _ = twice(lambda: point(False))
  assert patch_only == {'pSNR': distortion['pSNR_patches']}


def test_experiment_entry_points(device, scene):
  """The three names of the experiment script: training call, then the test
  call with what the training call returned."""
  from utils import quantization
  codes, patches, dictionary = (scene['codes'], scene['patches'],
                                scene['dictionary'])
  params = {'patch_dim': (8, 8), 'patch_positions': scene['positions']}
  widths = [2.0] * codes.shape[1]

  rate, dist, cbook, tab1, tab2 = twice(
      lambda: quantization.baseline_compute_RD_point(
          codes, patches, dictionary, quant_multiplier=2, binwidths=widths))
  assert tab1 is None and tab2 is None and set(dist) == {'pSNR'}
  test_rate, test_dist = twice(
      lambda: quantization.baseline_compute_RD_point(
          codes, patches, dictionary, precomputed_codebook=cbook,
          precomputed_huff_tab1=tab1, precomputed_huff_tab2=tab2,
          fullimg_reshape_params=params))
  assert test_rate == rate and set(test_dist) == {'pSNR', 'SSIM',
                                                  'pSNR_patches'}
  assert test_dist['pSNR_patches'] == dist['pSNR']

  rate_j, dist_j, cbook_j, ac, dc = twice(
      lambda: quantization.jpeg_compute_RD_point(
          codes, patches, dictionary, quant_multiplier=2, binwidths=widths))
  assert dist_j == dist and np.array_equal(cbook_j[0], cbook[0])
  test_rate, _ = twice(lambda: quantization.jpeg_compute_RD_point(
      codes, patches, dictionary, precomputed_codebook=cbook_j,
      precomputed_huff_tab_ac=ac, precomputed_huff_tab_dc=dc,
      fullimg_reshape_params=params))
  assert test_rate == rate_j

  rate_m, dist_m, fit, cw_len, tab = twice(
      lambda: quantization.Mod1_compute_RD_point(
          codes, patches, dictionary, quant_multiplier=2,
          init_binwidths=widths, max_iterations=8))
  assert tab is None and cw_len is fit['lengths']
  test_rate, test_dist = twice(lambda: quantization.Mod1_compute_RD_point(
      codes, patches, dictionary, quant_multiplier=2,
      precomputed_codebook=fit, precomputed_codebook_lengths=cw_len,
      precomputed_huff_tab1=tab, fullimg_reshape_params=params))
  assert test_rate == rate_m and test_dist['pSNR_patches'] == dist_m['pSNR']
