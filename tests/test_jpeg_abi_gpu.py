"""Every writing entry point of include/vtc_codec.h, three times over:

  fenced   tests/test_image_abi_fences_gpu.run_case as it is: a plain call,
           then inputs, outputs and workspace inside [guard | payload | guard]
           arenas (tests/fences.py), outputs and workspace 0xFF-filled, the
           workspace of EXACTLY the queried size; one byte less workspace must
           answer VTC_ERR_WORKSPACE and touch nothing
  skewed   the same run's third pass: every data pointer moved to its bare
           element alignment (4, 8 or 12 bytes past a 16-byte boundary for
           int32 / float32, 8 for the int64 / uint64 / double arrays, 3 for
           uint8)
  held     on a side stream behind a delay (tests/held_stream.py), every
           payload poisoned until the stream uploads the inputs, canaries on
           the null stream before and after the call, as tests/
           test_stream_order_gpu.py does for the other two headers

Each case is checked against tests/golden/jpeg.npz (the reference's symbols,
tables and streams; tools/make_jpeg_golden.py) or, for the quantiser, against
numpy in float64 -- exact equality throughout.  The shapes are the smallest
that still cross a 64-lane chunk: d = 3, s = 65; the offsets also run on 5000
rows, three tiles with a ragged last one.

CASES is imported as data by tests/test_jpeg_host.py, which fails when a
writing entry point of the header has no row here.  uint64 arrays travel as
their int64 bit patterns: torch moves bytes.
"""
import ctypes

import numpy as np
import pytest
import torch

import fences
import held_stream
import helpers
import test_image_abi_fences_gpu as image_table

pytestmark = pytest.mark.gpu

OK = 0
D, S = 3, 65
Case, Spec = image_table.Case, image_table.Spec

CASES = []


def case(entry, name):
  def deco(make):
    CASES.append(Case(entry, name, make))
    return make
  return deco


def _strings(array):
  return [b.decode('ascii') for b in array.tolist()]


def fixture_rows():
  """Three rows of the fixture's s = 65 case: a dense random row, the row with
  levels at 63 and 64 (neighbouring lanes of two chunks), the row whose only
  AC level is the last one; and the fixture's tables and streams for them."""
  from utils import jpeg
  g = helpers.load('jpeg')
  levels = g['levels_65']
  dense = int(np.argmax((levels != 0).sum(1)))
  edge = [i for i, r in enumerate(levels)
          if r[63] == 1 and r[64] == 2 and np.count_nonzero(r) == 2][0]
  last = [i for i, r in enumerate(levels)
          if r[64] == 3 and np.count_nonzero(r) == 1][0]
  rows = [dense, edge, last]
  tables = [dict(zip(_strings(g['table_%s_symbols_65' % kind]),
                     _strings(g['table_%s_codes_65' % kind])))
            for kind in ('ac', 'dc')]
  ac_code, ac_len = jpeg.table_arrays(tables[0], jpeg._AC_BYTE, 256)
  dc_code, dc_len = jpeg.table_arrays(tables[1], jpeg._DC_CATEGORY, 16)
  streams = [_strings(g['streams_65'])[i] for i in rows]
  ac = [g['ac_65'][g['ac_rows_65'][i]:g['ac_rows_65'][i + 1]] for i in rows]
  return {'levels': np.ascontiguousarray(levels[rows]), 'streams': streams,
          'ac': np.concatenate(ac), 'dc': g['dc_65'][rows],
          'ac_code': ac_code.view(np.int64), 'ac_len': ac_len,
          'dc_code': dc_code.view(np.int64), 'dc_len': dc_len}


def _quantize_case(with_order):
  def make(lib):
    rs = np.random.RandomState(65 + with_order)
    widths = 0.5 + 20 * rs.rand(S)
    codes = (rs.laplace(scale=40, size=(D, S))).astype(np.float32)
    codes[0, :4] = (np.array([0.5, 1.5, -2.5, 3.5]) * widths[:4]).astype(
        np.float32)
    order = rs.permutation(S).astype(np.int32)
    inputs = {'codes': codes, 'binwidths': widths}
    if with_order:
      inputs['order'] = order

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_jpeg_quantize(p['codes'], p['binwidths'],
                                   p.get('order'), p['levels'], D, S, stream)

    def truth(res, inputs):
      x = inputs['codes'].astype(np.float64)
      if with_order:
        x = x[:, order]
      assert np.array_equal(res['levels'], np.rint(x / widths))

    return Spec(inputs, {'levels': ((D, S), np.int32)}, call, truth)
  return make


case('vtc_jpeg_quantize', 'identity')(_quantize_case(0))
case('vtc_jpeg_quantize', 'order')(_quantize_case(1))


def _dequantize_case(with_order):
  def make(lib):
    rs = np.random.RandomState(75 + with_order)
    widths = 0.5 + 20 * rs.rand(S)
    levels = rs.randint(-300, 300, size=(D, S)).astype(np.int32)
    order = rs.permutation(S).astype(np.int32)
    inputs = {'levels': levels, 'binwidths': widths}
    if with_order:
      inputs['order'] = order

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_jpeg_dequantize(p['levels'], p['binwidths'],
                                     p.get('order'), p['codes'], D, S, stream)

    def truth(res, inputs):
      want = np.empty((D, S), dtype=np.float32)
      want[:, order if with_order else np.arange(S)] = (
          levels.astype(np.float64) * widths).astype(np.float32)
      assert np.array_equal(res['codes'], want)

    return Spec(inputs, {'codes': ((D, S), np.float32)}, call, truth)
  return make


case('vtc_jpeg_dequantize', 'identity')(_dequantize_case(0))
case('vtc_jpeg_dequantize', 'order')(_dequantize_case(1))


@case('vtc_jpeg_symbol_counts', 'd3-s65')
def _counts_case(lib):
  rows = fixture_rows()

  def call(lib, p, ws_ptr, ws_bytes, stream):
    return lib.vtc_jpeg_symbol_counts(p['levels'], D, S, p['ac_counts'],
                                      p['dc_counts'], p['status'], stream)

  def truth(res, inputs):
    assert np.array_equal(res['ac_counts'],
                          np.bincount(rows['ac'], minlength=256))
    assert np.array_equal(res['dc_counts'],
                          np.bincount(rows['dc'], minlength=16))
    assert res['status'].tolist() == [0, 0]

  return Spec({'levels': rows['levels']},
              {'ac_counts': ((256,), np.int64), 'dc_counts': ((16,), np.int64),
               'status': ((2,), np.int32)}, call, truth)


@case('vtc_jpeg_stream_bits', 'd3-s65')
def _bits_case(lib):
  rows = fixture_rows()

  def call(lib, p, ws_ptr, ws_bytes, stream):
    return lib.vtc_jpeg_stream_bits(p['levels'], D, S, p['ac_len'],
                                    p['dc_len'], p['bits'], p['status'],
                                    stream)

  def truth(res, inputs):
    assert res['bits'].tolist() == [len(x) for x in rows['streams']]
    assert res['status'].tolist() == [0, 0]

  return Spec({k: rows[k] for k in ('levels', 'ac_len', 'dc_len')},
              {'bits': ((D,), np.int32), 'status': ((2,), np.int32)}, call,
              truth)


def _offsets_case(d):
  def make(lib):
    bits = np.random.RandomState(d).randint(0, 5000, size=d).astype(np.int32)
    ws = lib.vtc_jpeg_bit_offsets_workspace_bytes(d)
    assert ws == 256

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_jpeg_bit_offsets(p['bits'], d, p['offsets'], ws_ptr,
                                      ws_bytes, stream)

    def truth(res, inputs):
      want = np.concatenate([[0], np.cumsum(bits.astype(np.int64))])
      assert np.array_equal(res['offsets'], want)

    return Spec({'bits': bits}, {'offsets': ((d + 1,), np.int64)}, call,
                truth, ws)
  return make


case('vtc_jpeg_bit_offsets', 'd3')(_offsets_case(3))
case('vtc_jpeg_bit_offsets', 'd5000')(_offsets_case(5000))


def _pack_case(missing_bytes):
  def make(lib):
    rows = fixture_rows()
    stream_bits = ''.join(rows['streams'])
    total = len(stream_bits)
    offsets = np.concatenate(
        [[0], np.cumsum([len(x) for x in rows['streams']])]).astype(np.int64)
    out_bytes = -(-total // 8) - missing_bytes
    assert out_bytes > 8

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_jpeg_pack(p['levels'], D, S, p['ac_code'], p['ac_len'],
                               p['dc_code'], p['dc_len'], p['offsets'],
                               p['out'], out_bytes, p['status'], stream)

    def truth(res, inputs):
      got = ''.join('1' if b else '0' for b in np.unpackbits(res['out']))
      kept = min(total, 8 * out_bytes)
      assert got[:kept] == stream_bits[:kept]
      assert set(got[kept:]) <= {'0'}
      assert res['status'].tolist() == [total - kept, 0]

    inputs = {k: rows[k] for k in ('levels', 'ac_code', 'ac_len', 'dc_code',
                                   'dc_len')}
    inputs['offsets'] = offsets
    return Spec(inputs, {'out': ((out_bytes,), np.uint8),
                         'status': ((2,), np.int32)}, call, truth)
  return make


case('vtc_jpeg_pack', 'exact-d3-s65')(_pack_case(0))
# out two and a bit bytes short of the total: the tail is dropped and counted
case('vtc_jpeg_pack', 'short-d3-s65')(_pack_case(3))

IDS = [c.id for c in CASES]


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_fenced_and_skewed(device, c):
  image_table.run_case(device, c)


# ------------------------------------------------------------ held stream
def _torch_dtype(np_dtype):
  return torch.from_numpy(np.zeros(1, np_dtype)).dtype


def _p(t):
  return ctypes.c_void_p(t.data_ptr())


def _plain(device, lib, spec, stream):
  t = {k: helpers.to_dev(v, device).clone() for k, v in spec.inputs.items()}
  for k, (shape, dtype) in spec.outputs.items():
    t[k] = torch.zeros(shape, dtype=_torch_dtype(dtype), device=device)
  ws = torch.zeros(2 * spec.ws_bytes + (1 << 20), dtype=torch.uint8,
                   device=device)
  pointers = {k: _p(v) for k, v in t.items()}
  torch.cuda.synchronize(device)
  rc, ms = held_stream.timed(
      lambda: spec.call(lib, pointers, _p(ws), ws.numel(), stream))
  torch.cuda.synchronize(device)
  assert rc == OK, 'plain: %s' % lib.vtc_last_error()
  return {k: t[k] for k in spec.outputs}, ms


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
    _plain(device, lib, spec, stream)
    largest = max(largest, _plain(device, lib, spec, stream)[1])
  h.set_delay(largest)
  print('jpeg_abi_delay %s' % h.describe())
  return h


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_held_side_stream(device, hold, c):
  import vtc_hip
  lib = vtc_hip.load_library()
  spec = c.make(lib)
  s = hold.streams[0]
  handle = ctypes.c_void_p(s.cuda_stream)
  assert s.cuda_stream != 0
  want, _ = _plain(device, lib, spec, vtc_hip.current_stream(device))

  t, f, pinned = {}, {}, {}
  for k, v in spec.inputs.items():
    t[k], f[k], pinned[k] = fences.fenced_staged(v, device)
  for k, (shape, dtype) in spec.outputs.items():
    t[k], f[k] = fences.fenced(shape, _torch_dtype(dtype), device)
  ws_ptr = ctypes.c_void_p(0)
  if spec.ws_bytes:
    ws, f['workspace'] = fences.fenced_workspace(spec.ws_bytes, device)
    ws_ptr = _p(ws)
  pointers = {k: _p(v) for k, v in t.items()}
  refill = [f[k] for k in spec.outputs] + (
      [f['workspace']] if spec.ws_bytes else [])
  source = t['levels' if 'levels' in spec.inputs else next(iter(spec.inputs))]
  word = np.ascontiguousarray(spec.inputs[
      'levels' if 'levels' in spec.inputs else next(iter(spec.inputs))])
  assert not (word.reshape(-1).view(np.uint8)[:4] == fences.POISON_BYTE).all()
  torch.cuda.synchronize(device)

  with torch.cuda.stream(s):
    hold.sleep()
    for fence in refill:
      fence.raw.fill_(fences.POISON_BYTE)
    for k, host in pinned.items():
      t[k].copy_(host.reshape(t[k].shape), non_blocking=True)
  before = held_stream.canary(source)
  rc, host_ms = held_stream.timed(
      lambda: spec.call(lib, pointers, ws_ptr, spec.ws_bytes, handle))
  after = held_stream.canary(source)
  s.synchronize()
  torch.cuda.synchronize(device)

  for label, canary in (('before', before), ('after', after)):
    assert held_stream.is_poison(canary), (
        '%s proved nothing: the null stream saw the staged input %s the call '
        '(%.3f ms on the host, delay %.1f ms): the delay was too short or the '
        'call synchronised' % (c.id, label, host_ms, hold.delay_ms))
  assert rc == OK, '%s held: status %d (%s)' % (c.id, rc,
                                                 lib.vtc_last_error())
  for k, fence in f.items():
    fence.assert_intact('%s (held): %s' % (c.id, k))
  for k in spec.inputs:
    assert torch.equal(t[k].cpu(), pinned[k].reshape(t[k].shape)), (
        '%s (held): input %s was modified' % (c.id, k))
  for k, v in want.items():
    if t[k].dtype.is_floating_point:
      f[k].assert_written('%s (held): %s' % (c.id, k))
    assert torch.equal(t[k], v), (
        '%s (held): %s differs from the default-stream call in %d of %d '
        'elements' % (c.id, k, int((t[k] != v).sum()), v.numel()))
  print('jpeg_abi_held %-40s delay_ms %.1f call_ms %.3f canaries ok'
        % (c.id, hold.delay_ms, host_ms))
