"""Every writing entry point of include/ext/vtc_jfif.h through raw ctypes, on
the pattern of tests/test_color_abi_gpu.py with the same runners as they are:

  fenced   tests/test_image_abi_fences_gpu.run_case: a plain call, then
           inputs, outputs and workspace inside [guard | payload | guard]
           arenas (tests/fences.py), outputs and workspace 0xFF-filled, the
           workspace of EXACTLY the queried size, and once more with every
           pointer at its bare element alignment (4 / 8 / 12 bytes for int32
           and float32, 8 for the 8-byte types, 2 for the uint16 tables, 3 for
           uint8); one byte less workspace answers VTC_ERR_WORKSPACE and
           touches nothing
  skewed1  every uint8 array -- raw, out, the length tables, table_sel -- one
           byte past a 16-byte boundary and every other array at its element
           size past one: what the byte kernels must survive
  held     on a side stream behind a delay (tests/held_stream.py), as
           tests/test_jpeg_abi_gpu.py does for vtc_codec.h

The rows: d = 1, and d = 37 (two workgroups of 32 rows, the second ragged)
laid out as the 4:2:0 scan of a 33 x 19 image plus one row.  The truth is the
restatement of tests/jfif_data.py, exact equality throughout.  uint16 arrays
travel as their int16 bit patterns, uint64 as int64: torch moves bytes.
"""
import ctypes

import numpy as np
import pytest
import torch

import fences
import jfif_data as truth
import test_image_abi_fences_gpu as image_table
import test_jpeg_abi_gpu as codec_table

pytestmark = pytest.mark.gpu

OK = 0
Case, Spec = image_table.Case, image_table.Spec
CASES = []


def case(entry, name):
  def deco(make):
    CASES.append(Case(entry, name, make))
    return make
  return deco


def _rows(d):
  """levels, pred, table_sel of d rows, the tokens and the tables the
  restatement builds for them, as device-ready arrays."""
  rs = np.random.RandomState(100 + d)
  _, pred, sel = truth.scan_arrays((33, 19), (2, 2))
  if d <= 36:
    pred, sel = pred[:d].copy(), sel[:d].copy()
  else:
    pred = np.concatenate([pred, [-1] * (d - 36)]).astype(np.int32)
    sel = np.concatenate([sel, [1] * (d - 36)]).astype(np.uint8)
  levels = (rs.randint(-60, 61, size=(d, 64)) *
            (rs.rand(d, 64) < 0.25)).astype(np.int32)
  levels[:, 0] = rs.randint(-300, 301, size=d)
  levels[0, 0] = 77      # the held-stream canary reads these four bytes
  levels[0, 1:] = 0
  levels[0, 40] = 1023                      # a run of 38: two ZRL, size 10
  levels[d - 1, 63] = -1                    # no end of block
  tokens = truth.scan_tokens(levels, pred, sel)
  ac, dc = truth.count_symbols(tokens)
  tables = truth.build_tables(ac, dc)
  arrays = {'ac_code': np.zeros((2, 256), np.uint16),
            'dc_code': np.zeros((2, 16), np.uint16),
            'ac_len': np.zeros((2, 256), np.uint8),
            'dc_len': np.zeros((2, 16), np.uint8)}
  for pair, table in enumerate(tables):
    if table is None:
      continue
    for key in ('ac', 'dc'):
      arrays[key + '_len'][pair] = table[key]
      for symbol, (code, _) in truth.canonical(table[key])[0].items():
        arrays[key + '_code'][pair, symbol] = code
  arrays['ac_code'] = arrays['ac_code'].view(np.int16)
  arrays['dc_code'] = arrays['dc_code'].view(np.int16)
  raw, nbits, offsets = truth.pack_tokens(tokens, tables)
  return {'levels': levels, 'pred': pred, 'table_sel': sel, 'ac': ac,
          'dc': dc, 'raw': raw, 'bits': np.diff(offsets).astype(np.int32),
          'offsets': offsets, 'arrays': arrays}


def _counts_case(d):
  def make(lib):
    rows = _rows(d)

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_jfif_symbol_counts(
          p['levels'], d, p['pred'], p['table_sel'], p['ac_counts'],
          p['dc_counts'], p['status'], stream)

    def check(res, inputs):
      assert np.array_equal(res['ac_counts'], rows['ac'])
      assert np.array_equal(res['dc_counts'], rows['dc'])
      assert res['status'].tolist() == [0, 0]

    return Spec({k: rows[k] for k in ('levels', 'pred', 'table_sel')},
                {'ac_counts': ((2, 256), np.int64),
                 'dc_counts': ((2, 16), np.int64),
                 'status': ((2,), np.int32)}, call, check)
  return make


def _bits_case(d):
  def make(lib):
    rows = _rows(d)

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_jfif_block_bits(
          p['levels'], d, p['pred'], p['table_sel'], p['ac_len'], p['dc_len'],
          p['bits'], p['status'], stream)

    def check(res, inputs):
      assert np.array_equal(res['bits'], rows['bits'])
      assert res['status'].tolist() == [0, 0]

    inputs = {k: rows[k] for k in ('levels', 'pred', 'table_sel')}
    inputs.update({k: rows['arrays'][k] for k in ('ac_len', 'dc_len')})
    return Spec(inputs, {'bits': ((d,), np.int32),
                         'status': ((2,), np.int32)}, call, check)
  return make


def _pack_case(d, missing_bytes):
  def make(lib):
    rows = _rows(d)
    total = int(rows['offsets'][-1])
    raw_bytes = len(rows['raw']) - missing_bytes
    assert raw_bytes >= 2

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_jfif_pack(
          p['levels'], d, p['pred'], p['table_sel'], p['ac_code'],
          p['ac_len'], p['dc_code'], p['dc_len'], p['offsets'], p['raw'],
          raw_bytes, p['status'], stream)

    def check(res, inputs):
      assert res['raw'].tobytes() == rows['raw'][:raw_bytes]
      padded = 8 * len(rows['raw'])           # stream bits and pad bits
      assert total <= padded < total + 8
      assert res['status'].tolist() == [padded - 8 * raw_bytes, 0]

    inputs = {k: rows[k] for k in ('levels', 'pred', 'table_sel', 'offsets')}
    inputs.update(rows['arrays'])
    return Spec(inputs, {'raw': ((raw_bytes,), np.uint8),
                         'status': ((2,), np.int32)}, call, check)
  return make


def _stuff_case(n, short):
  def make(lib):
    rs = np.random.RandomState(n)
    raw = rs.randint(0, 255, size=n).astype(np.uint8)
    raw[rs.rand(n) < 0.15] = 0xFF
    raw[0] = 0x12
    raw[[2047, 2048, n - 1]] = 0xFF
    want = truth.stuff(raw.tobytes())
    capacity = len(want) - short
    ws = lib.vtc_jfif_stuff_bytes_workspace_bytes(n)
    assert ws == 256 * -(-8 * -(-n // 2048) // 256)

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_jfif_stuff_bytes(p['raw'], n, p['out'], capacity,
                                      p['out_len'], p['status'], ws_ptr,
                                      ws_bytes, stream)

    def check(res, inputs):
      assert res['out'].tobytes() == want[:capacity]
      assert res['out_len'].tolist() == [len(want)]
      assert res['status'].tolist() == [short]

    return Spec({'raw': raw}, {'out': ((capacity,), np.uint8),
                               'out_len': ((1,), np.int64),
                               'status': ((1,), np.int32)}, call, check, ws)
  return make


H, W, BH, BW = 17, 23, 4, 3     # a block row that is padding only


def _dct_inputs():
  image = truth.gray_image(H, W)
  q = truth.quality_tables(75)[0]
  rob = np.random.RandomState(12).permutation(BH * BW).astype(np.int32)
  return image, q, rob


@case('vtc_jfif_forward_dct', '17x23-in-4x3')
def _forward_case(lib):
  image, q, rob = _dct_inputs()

  def call(lib, p, ws_ptr, ws_bytes, stream):
    return lib.vtc_jfif_forward_dct(p['plane'], H, W, BH, BW, p['basis'],
                                    p['q'], p['row_of_block'], p['levels'],
                                    BH * BW, stream)

  def check(res, inputs):
    want = truth.forward_dct(image, (BH, BW), q).reshape(BH * BW, 64)
    assert np.array_equal(res['levels'][rob], want)

  return Spec({'plane': image, 'basis': truth.basis(),
               'q': q.view(np.int16), 'row_of_block': rob},
              {'levels': ((BH * BW, 64), np.int32)}, call, check)


@case('vtc_jfif_inverse_dct', '17x23-in-4x3')
def _inverse_case(lib):
  image, q, rob = _dct_inputs()
  grid = truth.forward_dct(image, (BH, BW), q)
  levels = np.zeros((BH * BW, 64), dtype=np.int32)
  levels[rob] = grid.reshape(BH * BW, 64)

  def call(lib, p, ws_ptr, ws_bytes, stream):
    return lib.vtc_jfif_inverse_dct(p['levels'], BH * BW, p['row_of_block'],
                                    BH, BW, p['basis'], p['q'], p['plane'], H,
                                    W, stream)

  def check(res, inputs):
    assert truth.color_data.same_bits(
        res['plane'], truth.inverse_dct(grid, (H, W), q))

  return Spec({'levels': levels, 'row_of_block': rob, 'basis': truth.basis(),
               'q': q.view(np.int16)}, {'plane': ((H, W), np.float32)}, call,
              check)


for _d in (1, 37):
  case('vtc_jfif_symbol_counts', 'd%d' % _d)(_counts_case(_d))
  case('vtc_jfif_block_bits', 'd%d' % _d)(_bits_case(_d))
  case('vtc_jfif_pack', 'exact-d%d' % _d)(_pack_case(_d, 0))
# raw two bytes short of the segment: the tail is dropped and counted
case('vtc_jfif_pack', 'short-d37')(_pack_case(37, 2))
case('vtc_jfif_stuff_bytes', 'n4097-exact')(_stuff_case(4097, 0))
case('vtc_jfif_stuff_bytes', 'n4097-one-short')(_stuff_case(4097, 1))

IDS = [c.id for c in CASES]


def test_every_writing_entry_point_has_a_row():
  import vtc_hip
  writing = {name for name in vtc_hip.JFIF_BINDINGS
             if not name.endswith(('_abi_version', '_workspace_bytes'))}
  assert writing == {c.entry for c in CASES} and len(writing) == 6


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_fenced(device, c):
  image_table.run_case(device, c)


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_skewed_by_one_element(device, c):
  """uint8 arrays one byte past a 16-byte boundary, every other array one
  element past one; bitwise the plain call, guards intact."""
  import vtc_hip
  lib = vtc_hip.load_library()
  spec = c.make(lib)
  stream = vtc_hip.current_stream(device)
  want, _ = codec_table._plain(device, lib, spec, stream)
  spec.truth({k: v.cpu().numpy() for k, v in want.items()}, spec.inputs)

  t, f = {}, {}
  for k, v in spec.inputs.items():
    t[k], f[k] = fences.fenced_copy(v, device, skew=v.dtype.itemsize)
  for k, (shape, dtype) in spec.outputs.items():
    t[k], f[k] = fences.fenced(shape, codec_table._torch_dtype(dtype), device,
                               skew=np.dtype(dtype).itemsize)
  for k in ('raw', 'out', 'table_sel', 'ac_len', 'dc_len'):
    if k in t:
      assert t[k].data_ptr() % 16 == 1, k
  ws_ptr = ctypes.c_void_p(0)
  if spec.ws_bytes:
    ws, f['workspace'] = fences.fenced_workspace(spec.ws_bytes, device)
    ws_ptr = ctypes.c_void_p(ws.data_ptr())
  pointers = {k: ctypes.c_void_p(v.data_ptr()) for k, v in t.items()}
  rc = spec.call(lib, pointers, ws_ptr, spec.ws_bytes, stream)
  torch.cuda.synchronize(device)
  assert rc == OK, '%s skewed: %s' % (c.id, lib.vtc_last_error())
  for k, fence in f.items():
    fence.assert_intact('%s (+1 element): %s' % (c.id, k))
  for k, v in spec.inputs.items():
    assert np.array_equal(t[k].cpu().numpy(), v), k
  for k, v in want.items():
    assert torch.equal(t[k], v), (
        '%s (+1 element): %s differs from the plain call in %d elements'
        % (c.id, k, int((t[k] != v).sum())))


def test_null_pointers_and_bad_sizes_touch_nothing(device):
  """The refusals come before device work: the outputs keep their poison."""
  import vtc_hip
  lib = vtc_hip.load_library()
  stream = vtc_hip.current_stream(device)
  out, fence = fences.fenced((64,), torch.uint8, device)
  length, length_fence = fences.fenced((1,), torch.int64, device)
  status, status_fence = fences.fenced((2,), torch.int32, device)
  raw = torch.zeros(64, dtype=torch.uint8, device=device)
  p = lambda x: ctypes.c_void_p(x.data_ptr())
  null = ctypes.c_void_p(0)
  assert lib.vtc_jfif_stuff_bytes(null, 64, p(out), 64, p(length), p(status),
                                  null, 0, stream) == 1
  assert lib.vtc_jfif_stuff_bytes(p(raw), 64, p(out), 64, p(length),
                                  p(status), null, 0, stream) == 3
  assert lib.vtc_jfif_stuff_bytes(p(raw), -1, p(out), 64, p(length),
                                  p(status), null, 0, stream) == 1
  assert lib.vtc_jfif_pack(p(raw), 0, p(raw), p(raw), p(raw), p(raw), p(raw),
                           p(raw), p(raw), p(out), 64, p(status), stream) == 1
  assert lib.vtc_jfif_symbol_counts(p(raw), 1, p(raw), p(raw), null, p(raw),
                                    p(status), stream) == 1
  torch.cuda.synchronize(device)
  for name, fe in (('out', fence), ('out_len', length_fence),
                   ('status', status_fence)):
    fe.assert_intact(name)
    fe.assert_untouched(name)


# ------------------------------------------------------------ held stream
@pytest.fixture(scope='module')
def hold(device):
  """The shared delay, raised (never lowered) to ten times the slowest
  host-side enqueue of this table, each call timed on its second run."""
  import held_stream
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
  print('jfif_abi_delay %s' % h.describe())
  return h


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_held_side_stream(device, hold, c):
  codec_table.test_held_side_stream(device, hold, c)
