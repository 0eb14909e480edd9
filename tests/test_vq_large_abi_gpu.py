"""The three writing entry points of include/vtc_vq_large.h, three ways: the
table of tests/test_vq_abi_gpu.py (its runners as they are) at kmax = 4097,
the first size only this header takes, and at kmax = 40, where it has to
behave as the eighth does.

  fenced   tests/test_image_abi_fences_gpu.run_case: a plain call, then
           inputs, outputs and workspace inside [guard | payload | guard]
           arenas (tests/fences.py), outputs and workspace 0xFF-filled, the
           workspace of EXACTLY the queried size, every output element
           written; one byte less workspace must answer VTC_ERR_WORKSPACE and
           touch nothing
  skewed   float32 vectors 4, 8 and 12 bytes past a 16-byte boundary; the other
           4-byte arrays skewed by 4, the 8-byte arrays by 8
  held     on a side stream behind a delay (tests/held_stream.py), every
           payload poisoned until the stream uploads the inputs, canaries on
           the null stream before and after the call; bitwise the
           default-stream result

257 x 23 vectors; 33 codewords in use in kmax slots, the slots past them never
read.  The Lloyd step reads one state and writes another: the second step of a
fit from 40 codewords.  The truth is the numpy restatement of tests/vq_data.py.
"""
import ctypes

import numpy as np
import pytest

import held_stream
import test_image_abi_fences_gpu as image_table
import test_jpeg_abi_gpu as codec_table
import test_vq_abi_gpu as small_table
import vq_large_data as data

pytestmark = pytest.mark.gpu

B, D = 257, 23
KMAXES = (4097, 40)
IN_USE = 33        # codewords in use of the assignments
STEP_START = 40    # codewords the fit of the step starts from
LAM, EPSILON = 0.5, 1e-3
BOUND = 1e-11   # float64 sums of <= 257 terms: 257 * 2^-53 = 2.9e-14
Case, Spec = image_table.Case, image_table.Spec
STATE = small_table.STATE

CASES = []


def _vectors():
  return data.vectors(257, B, D)


def _book(kmax):
  """IN_USE codewords in kmax slots, +inf in the slots never read."""
  book = np.full((kmax, D), np.inf)
  book[:IN_USE] = data.initial_codebook(_vectors(), 128)[:IN_USE]
  return book


def _assign_case(kmax, lam, with_dequantized):
  def make(lib):
    x = _vectors()
    book = _book(kmax)
    k = np.array([IN_USE], np.int32)
    lengths = np.random.RandomState(40).uniform(1.0, 9.0, size=kmax)

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_vq_large_assign(
          p['vectors'], B, D, p['codebook'], p['lengths'] if lam else None,
          p['k'], kmax, lam, p['indices'],
          p['dequantized'] if with_dequantized else None, p['status'], stream)

    def truth(res, inputs):
      want, margin, _ = data.assign(inputs['vectors'], book, k, lengths, lam)
      assert margin > data.MARGIN
      assert np.array_equal(res['indices'], want)
      assert res['status'].tolist() == [0]
      if with_dequantized:
        assert np.array_equal(res['dequantized'],
                              data.base.dequantize(want, book))

    outputs = {'indices': ((B,), np.int32), 'status': ((1,), np.int64)}
    if with_dequantized:
      outputs['dequantized'] = ((B, D), np.float32)
    return Spec({'vectors': x, 'codebook': book, 'lengths': lengths, 'k': k},
                outputs, call, truth, 0)
  return make


def _second_step_input(kmax):
  """The state after the first step of a fit from STEP_START codewords in
  kmax slots."""
  x = _vectors()
  book = data.initial_codebook(x, 128)[:STEP_START]
  assert book.shape == (STEP_START, D)
  state, _ = data.base.initial_state(x, book)
  wide = {}
  for name, value in state.items():
    if name in ('codebook', 'lengths', 'counts'):
      wide[name] = np.zeros((kmax,) + value.shape[1:], value.dtype)
      wide[name][:STEP_START] = value
    else:
      wide[name] = value
  state, _ = data.step(x, wide, LAM, EPSILON, True)
  return x, state


def _step_case(kmax):
  def make(lib):
    import vtc_hip
    x, state = _second_step_input(kmax)
    ws = lib.vtc_vq_large_lloyd_step_workspace_bytes(B, D, kmax)
    assert ws == data.workspace_formula(B, D, kmax)
    inputs = {'vectors': x}
    inputs.update({'in_' + name: np.ascontiguousarray(state[name])
                   for name in STATE})

    def call(lib, p, ws_ptr, ws_bytes, stream):
      state_in = vtc_hip.VqState(**{name: p['in_' + name].value
                                    for name in STATE})
      state_out = vtc_hip.VqState(**{name: p[name].value for name in STATE})
      return lib.vtc_vq_large_lloyd_step(
          p['vectors'], B, D, kmax, LAM, EPSILON, 1, ctypes.byref(state_in),
          ctypes.byref(state_out), p['status'], ws_ptr, ws_bytes, stream)

    def truth(res, inputs):
      before = {name: inputs['in_' + name] for name in STATE}
      want, facts = data.step(inputs['vectors'], before, LAM, EPSILON, True)
      assert facts['margin'] > data.MARGIN and facts['convergence'] is not None
      assert res['status'].tolist() == [0]
      for name in data.base.STATE_INT:
        assert np.array_equal(res[name], want[name]), name
      assert want['k'][0] < before['k'][0] < STEP_START   # compacted twice
      assert not np.isnan(res['cost']).any()
      for name in data.base.STATE_FLOAT:
        assert np.array_equal(np.isinf(res[name]), np.isinf(want[name])), name
        ok = np.isfinite(want[name])
        scale = np.maximum(np.abs(want[name][ok]),
                           1.0 if name == 'lengths' else 0.0)
        assert (np.abs(res[name][ok] - want[name][ok]) <= BOUND * scale).all()

    outputs = {name: (state[name].shape, state[name].dtype) for name in STATE}
    outputs['status'] = ((1,), np.int64)
    return Spec(inputs, outputs, call, truth, ws)
  return make


def _counts_case(kmax):
  def make(lib):
    rs = np.random.RandomState(70)
    indices = rs.randint(-1, kmax + 1, size=B).astype(np.int32)
    indices[0] = 3   # the first word is no poison pattern
    indices[1] = kmax - 1

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_vq_large_index_counts(p['indices'], B, kmax, p['counts'],
                                           stream)

    def truth(res, inputs):
      assert np.array_equal(res['counts'],
                            data.index_counts(inputs['indices'], kmax))

    return Spec({'indices': indices}, {'counts': ((kmax,), np.int64)}, call,
                truth, 0)
  return make


for _kmax in KMAXES:
  CASES.append(Case('vtc_vq_large_assign',
                    '257x23-k%d-nearest-dequantized' % _kmax,
                    _assign_case(_kmax, 0.0, True)))
  CASES.append(Case('vtc_vq_large_assign', '257x23-k%d-lagrangian' % _kmax,
                    _assign_case(_kmax, LAM, False)))
  CASES.append(Case('vtc_vq_large_lloyd_step',
                    '257x23-k%d-second-step' % _kmax, _step_case(_kmax)))
  CASES.append(Case('vtc_vq_large_index_counts', '257-k%d' % _kmax,
                    _counts_case(_kmax)))

IDS = [c.id for c in CASES]


def test_every_writing_entry_point_has_a_row():
  import vtc_hip
  writing = {name for name in vtc_hip.VQ_LARGE_SIGNATURES
             if not name.endswith(('_workspace_bytes', '_abi_version'))}
  assert writing == {c.entry for c in CASES} and len(writing) == 3
  for kmax in KMAXES:
    assert {c.entry for c in CASES if '-k%d' % kmax in c.name} == writing
  assert max(KMAXES) == data.SMALL_MAX_CODEWORDS + 1
  assert min(KMAXES) <= data.SMALL_MAX_CODEWORDS


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_fenced(device, c):
  image_table.run_case(device, c)


SKEWED = [(c, skew) for c in CASES for skew in (4, 8, 12)]


@pytest.mark.parametrize('c,main_skew', SKEWED,
                         ids=['%s+%d' % (c.id, skew) for c, skew in SKEWED])
def test_skewed(device, c, main_skew):
  small_table.test_skewed(device, c, main_skew)


@pytest.fixture(scope='module')
def hold(device):
  """The shared delay, raised (never lowered) to ten times the slowest
  host-side enqueue of this table, each call timed on its second run."""
  import vtc_hip
  lib = vtc_hip.load_library()
  h = held_stream.hold(device)
  stream = vtc_hip.current_stream(device)
  largest = h.largest_enqueue_ms or 0.0
  for c in CASES:
    spec = c.make(lib)
    codec_table._plain(device, lib, spec, stream)
    largest = max(largest, codec_table._plain(device, lib, spec, stream)[1])
  h.set_delay(largest)
  print('vq_large_abi_delay %s' % h.describe())
  return h


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_held_side_stream(device, hold, c):
  codec_table.test_held_side_stream(device, hold, c)
