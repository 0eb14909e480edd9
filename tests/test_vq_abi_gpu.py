"""The three writing entry points of include/vtc_vq.h, three ways (modelled on
tests/test_quantization_abi_gpu.py, with the same runners as they are):

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

One shape, 257 x 23 vectors with kmax = 40 (rows past one workgroup of the
scan, the experiment's 23 components).  The Lloyd step reads one state and
writes another: the second step of a fit.  No row holds a NaN: an all-NaN input
answers a NaN cost, which the runners' torch.equal cannot compare
(test_every_row_nan_in_one_step of tests/test_vq_gpu.py makes that call
directly).  The truth is the numpy restatement of tests/vq_data.py, computed
here.
"""
import ctypes

import numpy as np
import pytest
import torch

import fences
import held_stream
import test_image_abi_fences_gpu as image_table
import test_jpeg_abi_gpu as codec_table
import vq_data as data

pytestmark = pytest.mark.gpu

OK = 0
B, D, KMAX = 257, 23, 40
LAM, EPSILON = 0.5, 1e-3
BOUND = 1e-11   # float64 sums of <= 257 terms: 257 * 2^-53 = 2.9e-14
Case, Spec = image_table.Case, image_table.Spec
STATE = ('codebook', 'lengths', 'counts', 'cost', 'k', 'zero_index', 'active',
         'iterations')

CASES = []


def case(entry, name):
  def deco(make):
    CASES.append(Case(entry, name, make))
    return make
  return deco


def padded(nbytes):
  return -(-nbytes // 256) * 256


def _vectors():
  return data.vectors(257, B, D)


def _quantiser():
  """33 codewords in 40 slots, the slots past them never read."""
  book = data.initial_codebook(_vectors(), 128)[:KMAX].copy()
  book[33:] = np.inf
  lengths = np.random.RandomState(40).uniform(1.0, 9.0, size=KMAX)
  return book, np.array([33], np.int32), lengths


def _assign_case(lam, with_dequantized):
  def make(lib):
    x = _vectors()
    book, k, lengths = _quantiser()

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_vq_assign(
          p['vectors'], B, D, p['codebook'], p['lengths'] if lam else None,
          p['k'], KMAX, lam, p['indices'],
          p['dequantized'] if with_dequantized else None, p['status'], stream)

    def truth(res, inputs):
      want, margin, _ = data.assign(inputs['vectors'], book, k, lengths, lam)
      assert margin > data.MARGIN
      assert np.array_equal(res['indices'], want)
      assert res['status'].tolist() == [0]
      if with_dequantized:
        assert np.array_equal(res['dequantized'], data.dequantize(want, book))

    outputs = {'indices': ((B,), np.int32), 'status': ((1,), np.int64)}
    if with_dequantized:
      outputs['dequantized'] = ((B, D), np.float32)
    return Spec({'vectors': x, 'codebook': book, 'lengths': lengths, 'k': k},
                outputs, call, truth, 0)
  return make


case('vtc_vq_assign', '257x23-nearest-dequantized')(_assign_case(0.0, True))
case('vtc_vq_assign', '257x23-lagrangian')(_assign_case(LAM, False))


def _second_step_input():
  """The state after the first step of a fit from 40 rows of the data."""
  x = _vectors()
  book = data.initial_codebook(x, 128)[:KMAX]
  assert book.shape == (KMAX, D)
  state, _ = data.initial_state(x, book)
  state, _ = data.step(x, state, LAM, EPSILON, True)
  return x, state


@case('vtc_vq_lloyd_step', '257x23-second-step')
def _step_case(lib):
  import vtc_hip
  x, state = _second_step_input()
  ws = lib.vtc_vq_lloyd_step_workspace_bytes(B, D, KMAX)
  assert ws == (padded(4 * B) + padded(8 * B) + padded(8 * KMAX * D) +
                padded(8 * KMAX) + padded(4 * KMAX) + padded(8 * KMAX) +
                padded(4 * KMAX) + 512)
  inputs = {'vectors': x}
  inputs.update({'in_' + name: np.ascontiguousarray(state[name])
                 for name in STATE})

  def call(lib, p, ws_ptr, ws_bytes, stream):
    state_in = vtc_hip.VqState(**{name: p['in_' + name].value
                                  for name in STATE})
    state_out = vtc_hip.VqState(**{name: p[name].value for name in STATE})
    return lib.vtc_vq_lloyd_step(
        p['vectors'], B, D, KMAX, LAM, EPSILON, 1, ctypes.byref(state_in),
        ctypes.byref(state_out), p['status'], ws_ptr, ws_bytes, stream)

  def truth(res, inputs):
    before = {name: inputs['in_' + name] for name in STATE}
    want, facts = data.step(inputs['vectors'], before, LAM, EPSILON, True)
    assert facts['margin'] > data.MARGIN and facts['convergence'] is not None
    assert res['status'].tolist() == [0]
    for name in data.STATE_INT:
      assert np.array_equal(res[name], want[name]), name
    assert want['k'][0] < before['k'][0] < KMAX     # compacted twice
    assert not np.isnan(res['cost']).any()
    for name in data.STATE_FLOAT:
      assert np.array_equal(np.isinf(res[name]), np.isinf(want[name])), name
      ok = np.isfinite(want[name])
      scale = np.maximum(np.abs(want[name][ok]),
                         1.0 if name == 'lengths' else 0.0)
      assert (np.abs(res[name][ok] - want[name][ok]) <= BOUND * scale).all()

  outputs = {name: (state[name].shape, state[name].dtype) for name in STATE}
  outputs['status'] = ((1,), np.int64)
  return Spec(inputs, outputs, call, truth, ws)


@case('vtc_vq_index_counts', '257-40')
def _counts_case(lib):
  rs = np.random.RandomState(70)
  indices = rs.randint(-1, KMAX + 1, size=B).astype(np.int32)
  indices[0] = 3   # the first word is no poison pattern

  def call(lib, p, ws_ptr, ws_bytes, stream):
    return lib.vtc_vq_index_counts(p['indices'], B, KMAX, p['counts'], stream)

  def truth(res, inputs):
    assert np.array_equal(res['counts'],
                          data.index_counts(inputs['indices'], KMAX))

  return Spec({'indices': indices}, {'counts': ((KMAX,), np.int64)}, call,
              truth, 0)


IDS = [c.id for c in CASES]


def test_every_writing_entry_point_has_a_row():
  import vtc_hip
  writing = {name for name in vtc_hip.VQ_SIGNATURES
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
    skew = main_skew if k in ('vectors', 'indices') else v.dtype.itemsize
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
  print('vq_abi_delay %s' % h.describe())
  return h


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_held_side_stream(device, hold, c):
  codec_table.test_held_side_stream(device, hold, c)
