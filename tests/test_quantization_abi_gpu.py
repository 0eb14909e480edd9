"""The three writing entry points of include/vtc_quant.h, three ways (modelled
on tests/test_code_stats_abi_gpu.py, with the same runners as they are):

  fenced   tests/test_image_abi_fences_gpu.run_case: a plain call, then
           inputs, outputs and workspace inside [guard | payload | guard]
           arenas (tests/fences.py), outputs and workspace 0xFF-filled, the
           workspace of EXACTLY the queried size, every output element
           written; one byte less workspace must answer VTC_ERR_WORKSPACE and
           touch nothing
  skewed   float32 codes 4, 8 and 12 bytes past a 16-byte boundary; the other
           4-byte arrays skewed by 4, the 8-byte arrays by 8
  held     on a side stream behind a delay (tests/held_stream.py), every
           payload poisoned until the stream uploads the inputs, canaries on
           the null stream before and after the call; bitwise the
           default-stream result

One shape, 257 x 70 codes with kmax = 40 (rows past one wave's rows, columns
past two 32-wide tiles).  The Lloyd step reads one state and writes another:
the second step of a fit, with one column frozen.  No column is all NaN: that
answers a NaN cost, which the runners' torch.equal cannot compare
(test_a_column_of_nan_codes_in_one_step of tests/test_quantization_gpu.py
makes that call directly).  The truth is the numpy restatement of
tests/quantization_data.py, computed here.
"""
import ctypes

import numpy as np
import pytest
import torch

import fences
import held_stream
import quantization_data as data
import test_image_abi_fences_gpu as image_table
import test_jpeg_abi_gpu as codec_table

pytestmark = pytest.mark.gpu

OK = 0
B, S, KMAX = 257, 70, 40
LAM, EPSILON = 0.05, 0.05   # the second step stops 14 of the 70 columns
BOUND = 1e-11   # float64 sums of <= 257 terms: 257 * 2^-53 = 2.9e-14
Case, Spec = image_table.Case, image_table.Spec
STATE = ('codebooks', 'lengths', 'counts', 'cost', 'k', 'zero_index', 'active',
         'iterations')

CASES = []


def case(entry, name):
  def deco(make):
    CASES.append(Case(entry, name, make))
    return make
  return deco


def padded(nbytes):
  return -(-nbytes // 256) * 256


def _codes():
  return data.codes(257, B, S)


def _quantiser():
  """33 codewords in 40 slots, every second column fewer."""
  books, k = data.grid_codebooks(S, KMAX, 0.375)
  k = np.where(np.arange(S) % 2, 33, 21).astype(np.int32)
  books = np.where(np.arange(KMAX)[None, :] < k[:, None], books, np.inf)
  lengths = np.random.RandomState(40).uniform(1.0, 9.0, size=(S, KMAX))
  return books, k, lengths


def _assign_case(lam, with_dequantized):
  def make(lib):
    x = _codes()
    books, k, lengths = _quantiser()

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_quant_assign(
          p['codes'], B, S, p['codebooks'], p['lengths'] if lam else None,
          p['k'], KMAX, lam, p['indices'],
          p['dequantized'] if with_dequantized else None, p['status'], stream)

    def truth(res, inputs):
      want, margin = data.assign(inputs['codes'], books, k, lengths, lam)
      assert margin > data.MARGIN
      assert np.array_equal(res['indices'], want)
      assert res['status'].tolist() == [0]
      if with_dequantized:
        assert np.array_equal(res['dequantized'],
                              data.dequantize(want, books))

    outputs = {'indices': ((B, S), np.int32), 'status': ((1,), np.int64)}
    if with_dequantized:
      outputs['dequantized'] = ((B, S), np.float32)
    return Spec({'codes': x, 'codebooks': books, 'lengths': lengths, 'k': k},
                outputs, call, truth, 0)
  return make


case('vtc_quant_assign', '257x70-nearest-dequantized')(_assign_case(0.0, True))
case('vtc_quant_assign', '257x70-lagrangian')(_assign_case(LAM, False))


def _second_step_input(pin_zero):
  """The state after the first step of a fit, one column frozen by hand."""
  x = _codes()
  books, k = data.grid_codebooks(S, KMAX, 0.375)
  state, _ = data.initial_state(x, books, k)
  state, _ = data.step(x, state, LAM, EPSILON, pin_zero)
  state['active'][5] = 0
  return x, state


@case('vtc_quant_lloyd_step', '257x70-second-step')
def _step_case(lib):
  import vtc_hip
  x, state = _second_step_input(True)
  ws = lib.vtc_quant_lloyd_step_workspace_bytes(B, S, KMAX)
  n = S * KMAX
  assert ws == 2 * padded(8 * n) + padded(4 * n)
  inputs = {'codes': x}
  inputs.update({'in_' + name: np.ascontiguousarray(state[name])
                 for name in STATE})

  def call(lib, p, ws_ptr, ws_bytes, stream):
    state_in = vtc_hip.QuantState(**{name: p['in_' + name].value
                                     for name in STATE})
    state_out = vtc_hip.QuantState(**{name: p[name].value for name in STATE})
    return lib.vtc_quant_lloyd_step(
        p['codes'], B, S, KMAX, LAM, EPSILON, 1, ctypes.byref(state_in),
        ctypes.byref(state_out), p['status'], ws_ptr, ws_bytes, stream)

  def truth(res, inputs):
    before = {name: inputs['in_' + name] for name in STATE}
    want, facts = data.step(inputs['codes'], before, LAM, EPSILON, True)
    assert facts['margin'] > data.MARGIN and facts['convergence']
    assert res['status'].tolist() == [0]
    for name in data.STATE_INT:
      assert np.array_equal(res[name], want[name]), name
    assert (want['k'] < before['k']).any()          # a column was compacted
    assert 0 < want['active'].sum() < S - 1         # some converged, some not
    assert not np.isnan(res['cost']).any()
    for name in data.STATE_FLOAT:
      assert np.array_equal(np.isinf(res[name]), np.isinf(want[name])), name
      ok = np.isfinite(want[name])
      scale = np.maximum(np.abs(want[name][ok]),
                         1.0 if name == 'lengths' else 0.0)
      assert (np.abs(res[name][ok] - want[name][ok]) <= BOUND * scale).all()
    for name in STATE:   # the frozen column, bit for bit
      assert np.array_equal(res[name][5], before[name][5]), name

  outputs = {name: (state[name].shape, state[name].dtype) for name in STATE}
  outputs['status'] = ((1,), np.int64)
  return Spec(inputs, outputs, call, truth, ws)


@case('vtc_quant_index_counts', '257x70-40')
def _counts_case(lib):
  rs = np.random.RandomState(70)
  indices = rs.randint(-1, KMAX + 1, size=(B, S)).astype(np.int32)
  indices[0, 0] = 3   # the first word is no poison pattern

  def call(lib, p, ws_ptr, ws_bytes, stream):
    return lib.vtc_quant_index_counts(p['indices'], B, S, KMAX, p['counts'],
                                      stream)

  def truth(res, inputs):
    assert np.array_equal(res['counts'],
                          data.index_counts(inputs['indices'], KMAX))

  return Spec({'indices': indices}, {'counts': ((S, KMAX), np.int64)}, call,
              truth, 0)


IDS = [c.id for c in CASES]


def test_every_writing_entry_point_has_a_row():
  import vtc_hip
  writing = {name for name in vtc_hip.QUANT_SIGNATURES
             if not name.endswith(('_workspace_bytes', '_abi_version'))}
  assert writing == {c.entry for c in CASES} and len(writing) == 3


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_fenced(device, c):
  image_table.run_case(device, c)


# --------------------------------------------------------- skewed pointers
SKEWED = [(c, skew) for c in CASES for skew in (4, 8, 12)]


@pytest.mark.parametrize('c,main_skew', SKEWED,
                         ids=['%s+%d' % (c.id, skew) for c, skew in SKEWED])
def test_skewed(device, c, main_skew):
  import vtc_hip
  lib = vtc_hip.load_library()
  spec = c.make(lib)
  stream = vtc_hip.current_stream(device)
  want, _ = codec_table._plain(device, lib, spec, stream)
  spec.truth({k: v.cpu().numpy() for k, v in want.items()}, spec.inputs)

  t, f = {}, {}
  for k, v in spec.inputs.items():
    skew = main_skew if k in ('codes', 'indices') else v.dtype.itemsize
    t[k], f[k] = fences.fenced_copy(v, device, skew=skew)
    assert t[k].data_ptr() % 16 == skew
  for k, (shape, dtype) in spec.outputs.items():
    skew = np.dtype(dtype).itemsize   # 4-byte arrays by 4, 8-byte arrays by 8
    t[k], f[k] = fences.fenced(shape, codec_table._torch_dtype(dtype), device,
                               skew=skew)
    assert t[k].data_ptr() % 16 == skew
  ws_ptr = ctypes.c_void_p(0)
  if spec.ws_bytes:
    ws, f['workspace'] = fences.fenced_workspace(spec.ws_bytes, device)
    ws_ptr = ctypes.c_void_p(ws.data_ptr())
  pointers = {k: ctypes.c_void_p(v.data_ptr()) for k, v in t.items()}
  rc = spec.call(lib, pointers, ws_ptr, spec.ws_bytes, stream)
  torch.cuda.synchronize(device)
  assert rc == OK, '%s skewed: %s' % (c.id, lib.vtc_last_error())
  for k, fence in f.items():
    fence.assert_intact('%s (+%d): %s' % (c.id, main_skew, k))
  for k, v in spec.inputs.items():
    assert np.array_equal(t[k].cpu().numpy(), v), k
  for k, v in want.items():
    if t[k].dtype.is_floating_point:
      f[k].assert_written('%s (+%d): %s' % (c.id, main_skew, k))
    assert torch.equal(t[k], v), (
        '%s (+%d): %s differs from the plain call in %d elements'
        % (c.id, main_skew, k, int((t[k] != v).sum())))


# ------------------------------------------------------------ held stream
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
  print('quantization_abi_delay %s' % h.describe())
  return h


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_held_side_stream(device, hold, c):
  codec_table.test_held_side_stream(device, hold, c)
