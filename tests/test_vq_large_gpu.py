"""The vector quantiser above 4096 codewords on the device
(include/vtc_vq_large.h, utils.vector_quantization with max_codewords) against
the entry points of include/vtc_vq.h where both apply -- byte for byte -- and
against the float64 numpy restatement of tests/vq_data.py above that.

Indices, counts, k, zero_index, iterations and active are EQUAL to the
restatement.  Codebook, lengths and cost are within the BOUND = 1e-11 of
tests/test_vq_gpu.py, whose derivation holds here: the largest float64 sums
run over the 8199 rows of one fit, 8199 * 2^-53 = 9.1e-13.  Every assignment
compared with the restatement has a margin above vq_data.MARGIN, no row and no
step is left out, and every call is made twice and compared bitwise.

The restatement of a fit from thousands of codewords costs 10-25 s of numpy;
each one is computed once, in a module-scoped fixture.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_quantization_gpu as scalar_tests
import test_vq_gpu as small_tests
import vq_data as small
import vq_large_data as data

pytestmark = pytest.mark.gpu

BOUND = small_tests.BOUND
STATE = small_tests.STATE
DEVICE_STATE = small_tests.DEVICE_STATE
LARGE = data.MAX_CODEWORDS
same_bits, twice, gap_of, dev = (scalar_tests.same_bits, scalar_tests.twice,
                                 scalar_tests.gap_of, scalar_tests.dev)
check_state, check_fit = small_tests.check_state, small_tests.check_fit
OLD, NEW = 'vtc_vq_', 'vtc_vq_large_'


# ------------------------------------------------------- the raw entry points
def raw_assign(device, prefix, x_dev, book, k, lengths, lam,
               with_dequantized=True):
  """<prefix>assign itself: `book` (kmax, d) and `lengths` [kmax] or None as
  they are, k the value of k[0].  Outputs start as 0xFF bytes."""
  import vtc_hip
  lib = vtc_hip.load_library()
  b, d = x_dev.shape
  book_dev = dev(book, device)
  lengths_dev = None if lengths is None else dev(lengths, device)
  k_dev = dev(np.array([k], np.int32), device)
  indices = torch.full((b,), -1, dtype=torch.int32, device=device)
  deq = torch.full((b, d), float('nan'), dtype=torch.float32, device=device)
  deq.view(torch.int32).fill_(-1)
  status = torch.full((1,), -1, dtype=torch.int64, device=device)
  vtc_hip.check(getattr(lib, prefix + 'assign')(
      vtc_hip.ptr(x_dev), b, d, vtc_hip.ptr(book_dev),
      vtc_hip.ptr(lengths_dev), vtc_hip.ptr(k_dev), book.shape[0], lam,
      vtc_hip.ptr(indices), vtc_hip.ptr(deq) if with_dequantized else None,
      vtc_hip.ptr(status), vtc_hip.current_stream(device)), prefix + 'assign')
  return indices, deq, status


def raw_counts(device, prefix, indices, kmax):
  import vtc_hip
  lib = vtc_hip.load_library()
  counts = torch.full((kmax,), -1, dtype=torch.int64, device=device)
  vtc_hip.check(getattr(lib, prefix + 'index_counts')(
      vtc_hip.ptr(indices), indices.shape[0], kmax, vtc_hip.ptr(counts),
      vtc_hip.current_stream(device)), prefix + 'index_counts')
  return counts


class Stepper(object):
  """A state on the device and <prefix>lloyd_step on it, in place or into a
  second state of 0xFF bytes; the workspace is of the queried size and starts
  as 0xFF bytes."""

  def __init__(self, device, prefix, x_dev, state):
    import vtc_hip
    self.hip, self.lib = vtc_hip, vtc_hip.load_library()
    self.device, self.prefix, self.x = device, prefix, x_dev
    self.state = {name: dev(state[name], device) for name in STATE}
    b, d = x_dev.shape
    self.kmax = state['codebook'].shape[0]
    self.ws_bytes = getattr(self.lib, prefix + 'lloyd_step_workspace_bytes')(
        b, d, self.kmax)
    assert self.ws_bytes > 0
    self.ws = vtc_hip.workspace(self.ws_bytes, device)

  def _struct(self, tensors):
    return self.hip.VqState(**{n: v.data_ptr() for n, v in tensors.items()})

  def step(self, lam, epsilon, pin_zero, in_place=True):
    """The state written (numpy) and status."""
    b, d = self.x.shape
    after = self.state
    if not in_place:
      after = {name: torch.full_like(value, -1)
               for name, value in self.state.items()}
      for name in small.STATE_FLOAT:
        after[name].view(torch.int64).fill_(-1)
    status = torch.full((1,), -1, dtype=torch.int64, device=self.device)
    self.ws.fill_(255)
    self.hip.check(getattr(self.lib, self.prefix + 'lloyd_step')(
        self.hip.ptr(self.x), b, d, self.kmax, lam, epsilon,
        1 if pin_zero else 0, ctypes.byref(self._struct(self.state)),
        ctypes.byref(self._struct(after)), self.hip.ptr(status),
        self.hip.ptr(self.ws), self.ws_bytes,
        self.hip.current_stream(self.device)), self.prefix + 'lloyd_step')
    out = {name: value.cpu().numpy() for name, value in after.items()}
    out['status'] = status.cpu().numpy()
    return out


def run_steps(device, prefix, x_dev, state, lam, epsilon, pin_zero, count):
  """The states after 1 .. count steps in place."""
  stepper = Stepper(device, prefix, x_dev, state)
  return [stepper.step(lam, epsilon, pin_zero) for _ in range(count)]


def assert_states_equal(got, want, label):
  for key in STATE + ('status',):
    assert same_bits(got[key], want[key]), (label, key)


# ------------------------------------------- 1. the same bits as the old path
def _small_cases():
  for name in sorted(small.FITS):
    yield name
  yield 'largest'


def _small_case(name):
  """(x, state, lambda for the steps, epsilon, pin_zero)."""
  if name == 'largest':      # test_the_largest_quantiser_in_one_step
    b, d, kmax = 2 * small.ASSIGN_ROWS + 3, 32, small.MAX_CODEWORDS
    rs = np.random.RandomState(43)
    state = {'codebook': small.random_codebook(42, kmax, d, scale=0.7),
             'lengths': rs.uniform(1.0, 12.0, kmax),
             'counts': np.zeros(kmax, np.int64),
             'cost': np.array([1e9, 0.0, 0.0]),
             'k': np.array([kmax], np.int32),
             'zero_index': np.array([0], np.int32),
             'active': np.ones(1, np.int32),
             'iterations': np.array([1], np.int32)}
    return small.vectors(41, b, d), state, 0.5, 1e-3, True
  lam, _, epsilon, pin_zero = small.FITS[name][4:]
  x, book = small.fit_inputs(name)
  state, _ = small.initial_state(x, book)
  return x, state, lam, epsilon, pin_zero


@pytest.mark.parametrize('name', list(_small_cases()))
def test_same_bits_as_the_small_entry_points(device, name):
  """kmax <= 4096: assign (lambda = 0 and != 0, with and without the
  dequantised rows), three steps in place and the index counts, every output
  array byte for byte that of the vtc_vq_* twin."""
  x, state, lam, epsilon, pin_zero = _small_case(name)
  x_dev = dev(x, device)
  book, lengths = state['codebook'], state['lengths']
  k, kmax = int(state['k'][0]), book.shape[0]
  assert kmax <= small.MAX_CODEWORDS
  for lam_assign, given, with_deq in ((0.0, None, True), (0.0, None, False),
                                      (0.5, lengths, True),
                                      (0.05, lengths, False)):
    old, new = [twice(lambda: raw_assign(device, prefix, x_dev, book, k, given,
                                         lam_assign, with_deq))
                for prefix in (OLD, NEW)]
    for a, c, what in zip(old, new, ('indices', 'dequantized', 'status')):
      assert same_bits(a, c), (name, lam_assign, what)
    assert (old[0] >= 0).all()
    counts = [twice(lambda: raw_counts(device, prefix, old[0], kmax))
              for prefix in (OLD, NEW)]
    assert same_bits(*counts), (name, lam_assign)
    assert int(counts[0].sum()) == len(x)
  old, new = [twice(lambda: run_steps(device, prefix, x_dev, state, lam,
                                      epsilon, pin_zero, 3))
              for prefix in (OLD, NEW)]
  for n, (a, c) in enumerate(zip(old, new)):
    assert_states_equal(c, a, '%s step %d' % (name, n + 1))
    assert a['status'].tolist() == [0]
  # and into a second state, the input left as it was
  apart = [twice(lambda: Stepper(device, prefix, x_dev, state).step(
      lam, epsilon, pin_zero, in_place=False)) for prefix in (OLD, NEW)]
  assert_states_equal(apart[1], apart[0], name + ' apart')
  assert_states_equal(apart[1], new[0], name + ' apart / in place')


# -------------------------------------------------- 2. indices past 16 bits
def test_indices_past_16_bits(device):
  """70 001 codewords of two components: 25 of the 515 rows land above index
  65 535, where an int16 (or uint16) staging of the indices would wrap."""
  from utils import vector_quantization as vq
  x = data.vectors(34, 515, 2, zero_rows=0.3, zeros=0.2)
  book = np.concatenate([np.zeros((1, 2)),
                         np.random.RandomState(5).laplace(size=(70000, 2)) *
                         0.7])
  kmax = len(book)
  want, margin, _ = data.assign(x, book, kmax)
  print('vq_large case 2: margin %.3g, %d rows above 65535'
        % (margin, (want > 65535).sum()))
  assert margin > data.MARGIN
  assert (want > 65535).sum() == 25
  x_dev = dev(x, device)
  indices, deq, status = twice(lambda: raw_assign(device, NEW, x_dev, book,
                                                  kmax, None, 0.0))
  assert np.array_equal(indices.cpu().numpy(), want)
  assert same_bits(deq.cpu().numpy(), small.dequantize(want, book))
  assert int(status) == 0
  counts = twice(lambda: raw_counts(device, NEW, indices, kmax))
  assert np.array_equal(counts.cpu().numpy(), data.index_counts(want, kmax))
  # the Python entry points
  got, got_deq = twice(lambda: vq.vector_assign(
      x_dev, book, return_dequantized=True, max_codewords=LARGE))
  assert same_bits(got, indices) and same_bits(got_deq, deq)
  assert same_bits(twice(lambda: vq.vector_index_counts(got, kmax, LARGE)),
                   counts)
  assert same_bits(twice(lambda: vq.vector_dequantize(got, book, LARGE)), deq)
  # with lengths: the same costs as numpy forms
  lengths = np.random.RandomState(6).uniform(1.0, 17.0, size=kmax)
  want, margin, _ = data.assign(x, book, kmax, lengths, 0.01)
  assert margin > data.MARGIN
  indices, _, _ = twice(lambda: raw_assign(device, NEW, x_dev, book, kmax,
                                           lengths, 0.01, False))
  assert np.array_equal(indices.cpu().numpy(), want)


# ------------------------------------------------------ 3 - 5. fits and steps
# name -> (seed, b, d, zero_rows, num_bins, lambda, steps)
LARGE_FITS = {
    'crossing': (38, 6149, 8, 0.0, 5000, 0.3, 3),
    'zero_cell': (39, 8199, 8, 0.2, 100000, 0.3, 3),
    'zero_cell_nearest': (39, 8199, 8, 0.2, 100000, 0.0, 3),
    'all_apart': (33, 4099, 23, 0.0, 4099, 0.05, 1),
}
EPSILON = 1e-3


def _large_fit(name):
  seed, b, d, zero_rows, num_bins, lam, count = LARGE_FITS[name]
  x = data.vectors(seed, b, d, zero_rows=zero_rows, zeros=0.2)
  book = data.initial_codebook(x, num_bins, LARGE)
  states, margin = data.steps(x, book, lam, EPSILON, True, count)
  ks = [int(s['k'][0]) for s in states]
  print('vq_large fit %s: k %s, smallest margin %.3g' % (name, ks, margin))
  assert margin > data.MARGIN, (name, margin)
  return {'x': x, 'book': book, 'states': states, 'k': ks, 'lam': lam}


@pytest.fixture(scope='module')
def crossing():
  fit = _large_fit('crossing')
  assert fit['k'] == [5001, 4582, 3963, 3406]
  return fit


@pytest.fixture(scope='module')
def zero_cell():
  fit = _large_fit('zero_cell')
  assert fit['k'] == [6536, 4288, 3983, 3962]
  zero = fit['states'][1]
  assert zero['counts'][zero['zero_index'][0]] > 0.15 * len(fit['x'])
  assert (fit['states'][0]['counts'] == 1).sum() > 4096   # singleton cells
  return fit


@pytest.fixture(scope='module')
def zero_cell_nearest():
  fit = _large_fit('zero_cell_nearest')
  assert fit['k'] == [fit['k'][0]] * 4 and fit['k'][0] > 6000
  return fit


@pytest.fixture(scope='module')
def all_apart():
  fit = _large_fit('all_apart')
  assert fit['k'] == [4100, 4100]
  # DP = 24, and a block of 2048 rows that sit in 2048 different cells
  assert fit['x'].shape[1] == 23
  assert (fit['states'][1]['counts'][1:] == 1).all()
  return fit


def check_steps(device, fit, label):
  """Every step of the fit on the device, in place, against the restatement;
  then vector_lloyd from the same start."""
  from utils import vector_quantization as vq
  x_dev = dev(fit['x'], device)
  want, lam = fit['states'], fit['lam']
  count = len(want) - 1
  got = twice(lambda: run_steps(device, NEW, x_dev, want[0], lam, EPSILON,
                                True, count))
  for n in range(count):
    for key in ('active', 'iterations'):
      assert np.array_equal(got[n][key], want[n + 1][key]), (label, n, key)
    assert got[n]['status'].tolist() == [0]
    check_state(got[n], want[n + 1], '%s_step%d' % (label, n + 1))
    knew = int(want[n + 1]['k'][0])
    assert (got[n]['codebook'][knew:] == 0).all()
    assert (got[n]['lengths'][knew:] == 0).all()
    assert (got[n]['counts'][knew:] == 0).all()
  start = twice(lambda: vq.initial_vector_codebook(
      x_dev, LARGE_FITS[label][4], max_codewords=LARGE))
  assert same_bits(start.cpu().numpy(), fit['book'])
  result = twice(lambda: vq.vector_lloyd(
      x_dev, start, lagrange_mult=lam, max_iterations=count, epsilon=EPSILON,
      max_codewords=LARGE))
  assert result['codebook'].shape == fit['book'].shape
  check_fit(result, want[-1], label + '_fit')
  for key in DEVICE_STATE:      # the fit is those steps
    assert same_bits(result[key].cpu().numpy(), got[-1][key]), (label, key)
  return result


def test_a_fit_that_starts_above_4096_cells_and_crosses_it(device, crossing):
  check_steps(device, crossing, 'crossing')


def test_a_big_zero_cell_with_many_singleton_cells(device, zero_cell):
  check_steps(device, zero_cell, 'zero_cell')


def test_nearest_codeword_keeps_every_cell(device, zero_cell_nearest):
  check_steps(device, zero_cell_nearest, 'zero_cell_nearest')


def test_a_block_whose_rows_all_sit_in_different_cells(device, all_apart):
  check_steps(device, all_apart, 'all_apart')


# ------------------------------------------------------------------ 6. edges
EDGE_KMAX = small.MAX_CODEWORDS + 1


def _edge_quantiser(d, seed=7):
  book = small.random_codebook(seed, EDGE_KMAX, d)
  lengths = np.random.RandomState(seed).uniform(1.0, 9.0, size=EDGE_KMAX)
  return book, lengths


def _edge_state(book, lengths, k, active=1, iterations=2):
  return {'codebook': book, 'lengths': lengths,
          'counts': np.arange(len(book), dtype=np.int64),
          'cost': np.array([1e9, 2.0, 1.0]), 'k': np.array([k], np.int32),
          'zero_index': np.array([0], np.int32),
          'active': np.array([active], np.int32),
          'iterations': np.array([iterations], np.int32)}


def test_k_of_one_and_k_above_kmax(device):
  x = small.vectors(51, 300, 5, scale=2.0)
  x_dev = dev(x, device)
  book, lengths = _edge_quantiser(5)
  for k, used in ((1, 1), (EDGE_KMAX + 9, EDGE_KMAX), (0, 1), (-4, 1)):
    want, margin, _ = data.assign(x, book, used, lengths, 0.05)
    assert margin > data.MARGIN or used == 1
    indices, deq, status = twice(lambda: raw_assign(
        device, NEW, x_dev, book, k, lengths, 0.05))
    assert np.array_equal(indices.cpu().numpy(), want), k
    assert same_bits(deq.cpu().numpy(), small.dequantize(want, book))
    assert int(status) == 0
  # a step with k above kmax: clamped before any read
  state = _edge_state(book, lengths, EDGE_KMAX)
  want, facts = data.step(x, state, 0.05, 1e-3, True)
  assert facts['margin'] > data.MARGIN and facts['lost'] > 3000
  state['k'] = np.array([EDGE_KMAX + 9], np.int32)
  got = twice(lambda: run_steps(device, NEW, x_dev, state, 0.05, 1e-3, True,
                                1))[0]
  for key in ('active', 'iterations'):
    assert np.array_equal(got[key], want[key]), key
  check_state(got, want, 'clamped')


def test_nan_rows(device):
  from utils import vector_quantization as vq
  d = 5
  x = small.vectors(52, small.ASSIGN_ROWS + 3, d, scale=2.0)
  x[3, 1] = np.nan
  x[64, :] = np.nan
  x[256, 0] = np.nan
  book, lengths = _edge_quantiser(d)
  x_dev = dev(x, device)
  want, margin, _ = data.assign(x, book, EDGE_KMAX)
  assert margin > data.MARGIN and (want < 0).sum() == 3
  indices, deq, status = twice(lambda: raw_assign(device, NEW, x_dev, book,
                                                  EDGE_KMAX, None, 0.0))
  assert np.array_equal(indices.cpu().numpy(), want)
  assert int(status) == 3
  got = deq.cpu().numpy()
  assert np.array_equal(np.isnan(got), np.repeat((want < 0)[:, None], d, 1))
  assert same_bits(got[want >= 0], small.dequantize(want, book)[want >= 0])
  counts = twice(lambda: raw_counts(device, NEW, indices, EDGE_KMAX))
  assert np.array_equal(counts.cpu().numpy(),
                        data.index_counts(want, EDGE_KMAX))
  # a step counts them and leaves them out of every cell
  state = _edge_state(book, lengths, EDGE_KMAX)
  want_state, facts = data.step(x, state, 0.05, 1e-3, True)
  assert facts['margin'] > data.MARGIN
  got = twice(lambda: run_steps(device, NEW, x_dev, state, 0.05, 1e-3, True,
                                1))[0]
  assert got['status'].tolist() == [3]
  check_state(got, want_state, 'nan_rows')
  with pytest.raises(ValueError, match='NaN'):
    vq.vector_lloyd(x_dev, book, max_iterations=2, max_codewords=LARGE)


def test_an_inactive_state_is_copied_bit_for_bit(device):
  """active == 0: all kmax slots of every array as they were, whatever they
  hold, and status 0 although a row is NaN."""
  rs = np.random.RandomState(12)
  d = 23
  x = small.vectors(12, 300, d)
  x[5, 1] = np.nan
  state = {'codebook': rs.randn(EDGE_KMAX, d),
           'lengths': rs.uniform(1, 9, EDGE_KMAX),
           'counts': rs.randint(0, 99, EDGE_KMAX).astype(np.int64),
           'cost': np.array([3.0, 2.0, 1.0]), 'k': np.array([33], np.int32),
           'zero_index': np.array([-1], np.int32),
           'active': np.zeros(1, np.int32),
           'iterations': np.array([7], np.int32)}
  state['codebook'][4000:] = np.nan            # never read, copied all the same
  for in_place in (False, True):
    got = twice(lambda: Stepper(device, NEW, dev(x, device), state).step(
        0.5, 1e-3, True, in_place=in_place))
    for key in STATE:
      assert same_bits(got[key], np.ascontiguousarray(state[key])), key
    assert got['status'].tolist() == [0]


def test_every_row_nan_in_one_step(device):
  b, d = 70, 5
  x = np.full((b, d), np.nan, np.float32)
  x[:, 1::2] = 1.0
  book, lengths = _edge_quantiser(d)
  state = _edge_state(book, lengths, 4000)
  want, _ = data.step(x, state, 0.5, 1e-3, True)
  assert np.isnan(want['cost']).all() and want['active'][0] == 0
  got = twice(lambda: Stepper(device, NEW, dev(x, device), state).step(
      0.5, 1e-3, True, in_place=False))
  for key in DEVICE_STATE:
    assert same_bits(got[key], np.ascontiguousarray(state[key])), key
  assert np.isnan(got['cost']).all()
  assert got['active'].tolist() == [0] and got['iterations'].tolist() == [3]
  assert got['status'].tolist() == [b]


def test_pin_zero_off_and_one_row(device):
  """Without the pin the zero cell is a cell like the others: its codeword
  moves to the mean of its members, or goes when it has none; b = 1."""
  d = 5
  book, lengths = _edge_quantiser(d)
  # rows near the zero vector but not on it: the unpinned zero cell moves
  x = (np.random.RandomState(53).laplace(size=(300, d)) * 0.05).astype(
      np.float32)
  for pin_zero in (False, True):
    state = _edge_state(book, lengths, EDGE_KMAX)
    want, facts = data.step(x, state, 0.05, 1e-3, pin_zero)
    assert facts['margin'] > data.MARGIN
    assert (want['zero_index'][0] >= 0) == pin_zero
    got = twice(lambda: run_steps(device, NEW, dev(x, device), state, 0.05,
                                  1e-3, pin_zero, 1))[0]
    for key in ('active', 'iterations'):
      assert np.array_equal(got[key], want[key]), key
    check_state(got, want, 'pin_%d' % pin_zero)
  # far from the zero vector: unpinned it has no member and is dropped
  x = small.vectors(54, 1, d, zero_rows=0.0, zeros=0.0, scale=2.0)
  assert x.shape == (1, d)
  for pin_zero in (False, True):
    state = _edge_state(book, lengths, EDGE_KMAX)
    want, facts = data.step(x, state, 0.0, 1e-3, pin_zero)
    assert facts['margin'] > data.MARGIN
    assert int(want['k'][0]) == (2 if pin_zero else 1)
    got = twice(lambda: run_steps(device, NEW, dev(x, device), state, 0.0,
                                  1e-3, pin_zero, 1))[0]
    check_state(got, want, 'one_row_pin_%d' % pin_zero)
    indices, _, _ = twice(lambda: raw_assign(device, NEW, dev(x, device),
                                             book, EDGE_KMAX, None, 0.0))
    assert np.array_equal(indices.cpu().numpy(),
                          data.assign(x, book, EDGE_KMAX)[0])


# -------------------------------------------------------- 7. Python surface
def test_routing_by_kmax(device):
  """kmax <= 4096: the old entry points whatever max_codewords says;
  4096 < kmax <= max_codewords: the large ones; above: NotImplementedError
  naming the limit in force."""
  from utils import vector_quantization as vq
  x = small.vectors(55, 300, 3, scale=2.0)
  x_dev = dev(x, device)
  book = small.random_codebook(56, 5000, 3)
  small_book = book[:4096]
  for limit in (4096, 5000, LARGE):
    got = twice(lambda: vq.vector_assign(x_dev, small_book,
                                         max_codewords=limit))
    assert same_bits(got, vq.vector_assign(x_dev, small_book))
  want, margin, _ = data.assign(x, book, 5000)
  assert margin > data.MARGIN
  for limit in (5000, LARGE):
    got = twice(lambda: vq.vector_assign(x_dev, book, max_codewords=limit))
    assert np.array_equal(got.cpu().numpy(), want)
  indices = vq.vector_assign(x_dev, book, max_codewords=5000)
  for limit, word in ((None, 'at most 4096'), (4096, 'at most 4096'),
                      (4999, 'at most 4999')):
    kwargs = {} if limit is None else {'max_codewords': limit}
    with pytest.raises(NotImplementedError, match=word):
      vq.vector_assign(x_dev, book, **kwargs)
    with pytest.raises(NotImplementedError, match=word):
      vq.vector_lloyd(x_dev, book, max_iterations=1, **kwargs)
    with pytest.raises(NotImplementedError, match=word):
      vq.vector_index_counts(indices, 5000, **kwargs)
    with pytest.raises(NotImplementedError, match=word):
      vq.vector_dequantize(indices, book, **kwargs)
  with pytest.raises(NotImplementedError, match='at most %d' % LARGE):
    vq.vector_assign(x_dev, np.zeros((LARGE + 1, 3)), max_codewords=LARGE)
  with pytest.raises(ValueError, match='max_codewords'):
    vq.vector_assign(x_dev, book, max_codewords=LARGE + 1)
  # a small fit under a large limit is the fit of today, bit for bit
  start = vq.initial_vector_codebook(x_dev, 64)
  assert same_bits(start, vq.initial_vector_codebook(x_dev, 64,
                                                     max_codewords=LARGE))
  scalar_tests.assert_same(
      vq.vector_lloyd(x_dev, start, 0.05, max_iterations=3),
      vq.vector_lloyd(x_dev, start, 0.05, max_iterations=3,
                      max_codewords=LARGE))


def test_trim_and_the_table_codes(device, crossing):
  """The fit of case 3 ends at 3406 codewords in 5001 slots.  Trimmed, it
  assigns exactly as before and the Huffman and range coders take it; as it is
  they refuse it and name trim_vector_codebook."""
  from utils import vector_quantization as vq
  x = crossing['x']
  x_dev = dev(x, device)
  lam = crossing['lam']
  result = vq.vector_lloyd(x_dev, crossing['book'], lagrange_mult=lam,
                           max_iterations=3, epsilon=EPSILON,
                           max_codewords=LARGE)
  trimmed = twice(lambda: vq.trim_vector_codebook(result))
  k = crossing['k'][-1]
  assert k <= small.MAX_CODEWORDS < result['codebook'].shape[0]
  assert trimmed['codebook'].shape == (k, x.shape[1])
  assert trimmed['lengths'].shape == (k,) and trimmed['counts'].shape == (k,)
  assert int(trimmed['k']) == k
  for key in ('codebook', 'lengths', 'counts'):
    assert same_bits(trimmed[key], result[key][:k]), key
  for key in ('zero_index', 'iterations', 'converged', 'cost'):
    scalar_tests.assert_same(trimmed[key], result[key], key)
  whole = twice(lambda: vq.vector_assign(
      x_dev, result, lagrange_mult=lam, return_dequantized=True,
      max_codewords=LARGE))
  cut = twice(lambda: vq.vector_assign(x_dev, trimmed, lagrange_mult=lam,
                                       return_dequantized=True))
  scalar_tests.assert_same(whole, cut)
  want, margin, _ = data.assign(
      x, result['codebook'].cpu().numpy(), k,
      result['lengths'].cpu().numpy(), lam)
  assert margin > data.MARGIN
  assert np.array_equal(cut[0].cpu().numpy(), want)

  # one scalar column in front of the eight of the vector
  rs = np.random.RandomState(57)
  scalar = np.rint(rs.laplace(size=(len(x), 1)) * 3).astype(np.float32)
  codes = dev(np.concatenate([scalar, x], 1), device)
  dictionary = dev(rs.randn(9, 12).astype(np.float32), device)
  patches = codes @ dictionary
  scal = vq.uniform_codebooks([scalar.min()], [scalar.max()], [1.0])
  vec_clust = list(range(1, 9))

  def point(book, **kwargs):
    return vq.compute_RD_point_mixed(codes, patches, dictionary, [0], scal,
                                     vec_clust, book, vec_lagrange_mult=lam,
                                     **kwargs)
  entropy = twice(lambda: point(trimmed))
  uncut = twice(lambda: point(result, vec_max_codewords=LARGE))
  assert uncut[1] == entropy[1]
  assert abs(uncut[0] - entropy[0]) <= 1e-12 * entropy[0]
  for source_code in ('huffman', 'ans'):
    with pytest.raises(NotImplementedError, match='trim_vector_codebook'):
      point(result, source_code=source_code, vec_max_codewords=LARGE)
    rate, dist, tables = twice(lambda: point(trimmed,
                                             source_code=source_code))
    assert dist == entropy[1]
    assert entropy[0] <= rate <= entropy[0] * 1.1 + 2.0 / patches.shape[1], (
        source_code, rate, entropy[0])
    rate_s, dist_s, _ = twice(lambda: point(trimmed, source_code=source_code,
                                            tables=tables, from_stream=True))
    assert dist_s == dist and rate_s >= rate


@pytest.fixture(scope='module')
def rd_scene():
  s = data.scene()
  want = data.mod3_point(s, LARGE)
  print('vq_large rd: k %d of kmax %d, margin %.3g, rate %.6f'
        % (want['vec']['k'][0], want['vec']['codebook'].shape[0],
           want['margin'], want['rate']))
  assert want['margin'] > data.MARGIN
  assert want['vec']['codebook'].shape[0] > small.MAX_CODEWORDS
  return s, want


def test_mod3_point_from_100000_bins(device, rd_scene):
  """The experiment's call, vec_init_num_bins = 100000, with
  vec_max_codewords = 131072 on a scene of more than 4096 distinct tail
  vectors: the rate within 1e-12 relative of the restatement's and the
  distortion that of the restatement's dequantised codes, the tolerances of
  test_experiment_entry_points of tests/test_vq_gpu.py.  Without the keyword
  the call is today's: 4096 candidates."""
  from utils import quantization
  from utils import vector_quantization as vq
  s, want = rd_scene
  codes, patches, dictionary = (dev(s[key], device) for key in
                                ('codes', 'patches', 'dictionary'))
  widths = [small.SCAL_WIDTH] * len(small.SCAL_CLUSTS)

  def train(**kwargs):
    return vq.Mod3_compute_RD_point(
        codes, patches, dictionary, small.SCAL_CLUSTS, small.VEC_CLUST,
        scal_quant_multiplier=data.RD_SCAL_MULT, scal_binwidths=widths,
        vec_quant_multiplier=data.RD_VEC_MULT, vec_init_num_bins=100000,
        max_iterations=data.RD_ITERATIONS, epsilon=data.RD_EPSILON, **kwargs)
  out = twice(lambda: train(vec_max_codewords=LARGE))
  assert len(out) == 8 and out[5:] == (None, None, None)
  rate, dist, scal_cbook, vec_cbook, vec_cw_len = out[:5]
  assert vec_cw_len is vec_cbook['lengths'] and set(dist) == {'pSNR'}
  got_vec = {key: vec_cbook[key].cpu().numpy() for key in DEVICE_STATE}
  got_vec['cost'] = want['vec']['cost']
  check_state(got_vec, want['vec'], 'mod3_vec')
  print('vq_large rd rate %.9f restatement %.9f pSNR %.6f restatement %.6f'
        % (rate, want['rate'], dist['pSNR'], want['psnr_patches']))
  assert abs(rate - want['rate']) <= 1e-12 * want['rate']
  back = quantization._reconstruct(dev(want['dequantized'], device),
                                   dictionary)
  assert dist == quantization._distortion(patches, back, None)
  assert abs(dist['pSNR'] - want['psnr_patches']) <= 1e-4
  # the test call with what the training call returned
  test_rate, test_dist = twice(lambda: vq.Mod3_compute_RD_point(
      codes, patches, dictionary, small.SCAL_CLUSTS, small.VEC_CLUST,
      vec_quant_multiplier=data.RD_VEC_MULT,
      precomputed_scal_codebook=scal_cbook,
      precomputed_vec_codebook=vec_cbook,
      precomputed_vec_codebook_lengths=vec_cw_len, vec_max_codewords=LARGE))
  assert test_rate == rate and test_dist == dist
  with pytest.raises(NotImplementedError, match='at most 4096'):
    vq.Mod3_compute_RD_point(
        codes, patches, dictionary, small.SCAL_CLUSTS, small.VEC_CLUST,
        vec_quant_multiplier=data.RD_VEC_MULT,
        precomputed_scal_codebook=scal_cbook,
        precomputed_vec_codebook=vec_cbook,
        precomputed_vec_codebook_lengths=vec_cw_len)
  # a table code: the training call cuts its fit down to the slots in use
  k = int(want['vec']['k'][0])
  assert k <= small.MAX_CODEWORDS < vec_cbook['codebook'].shape[0]
  for source_code in ('huffman', 'ans'):
    coded = twice(lambda: train(vec_max_codewords=LARGE,
                                source_code=source_code))
    assert coded[3]['codebook'].shape[0] == k and coded[4] is coded[3][
        'lengths']
    for key in ('codebook', 'lengths', 'counts'):
      assert same_bits(coded[3][key], vec_cbook[key][:k]), key
    assert coded[1] == dist and coded[0] >= rate
    assert coded[5] is not None and coded[6] is not None
    with pytest.raises(NotImplementedError, match='trim_vector_codebook'):
      vq.Mod3_compute_RD_point(
          codes, patches, dictionary, small.SCAL_CLUSTS, small.VEC_CLUST,
          vec_quant_multiplier=data.RD_VEC_MULT,
          precomputed_scal_codebook=scal_cbook,
          precomputed_vec_codebook=vec_cbook,
          precomputed_vec_codebook_lengths=vec_cw_len,
          precomputed_huff_tab1=coded[5], precomputed_huff_tab2=coded[6],
          source_code=source_code, vec_max_codewords=LARGE)
  # without the keyword: today's call, and the keyword at 4096 is that call
  today = twice(lambda: train())
  explicit = train(vec_max_codewords=small.MAX_CODEWORDS)
  scalar_tests.assert_same(today, explicit)
  start = small.initial_codebook(s['codes'][:, small.VEC_CLUST], 100000)
  assert today[3]['codebook'].shape[0] == len(start) <= small.MAX_CODEWORDS
  assert same_bits(
      vq.initial_vector_codebook(codes[:, small.VEC_CLUST].contiguous(),
                                 100000).cpu().numpy(), start)
  # Mod2 takes the keyword the same way
  mod2 = twice(lambda: vq.Mod2_compute_RD_point(
      codes, patches, dictionary, small.SCAL_CLUSTS, small.VEC_CLUST,
      scal_quant_multiplier=data.RD_SCAL_MULT, scal_binwidths=widths,
      vec_quant_multiplier=data.RD_VEC_MULT, vec_init_num_bins=100000,
      max_iterations=data.RD_ITERATIONS, epsilon=data.RD_EPSILON,
      vec_max_codewords=LARGE))
  for key in DEVICE_STATE:      # the vector part does not depend on the scalars
    assert same_bits(mod2[3][key], vec_cbook[key]), key
