"""vtc_jpeg_unpack, the writing entry point of include/vtc_decode.h, three ways
(modelled on tests/test_jpeg_abi_gpu.py, whose runners it calls):

  fenced   tests/test_image_abi_fences_gpu.run_case as it is: a plain call,
           then inputs, outputs and workspace inside [guard | payload | guard]
           arenas (tests/fences.py), outputs and workspace 0xFF-filled, the
           workspace of EXACTLY the queried size; one byte less workspace must
           answer VTC_ERR_WORKSPACE and touch nothing
  skewed   `packed` 1, 2 and 3 bytes past a 16-byte boundary, `levels` 4,
           `offsets`, `status` and the two code arrays 8, the length arrays 3
  held     on a side stream behind a delay (tests/held_stream.py), every
           payload poisoned until the stream uploads the inputs, canaries on
           the null stream before and after the call

The truth is tests/golden/jpeg.npz: the reference's streams, packed behind
three bits that belong to no row, decode to the reference's levels.  The
cases: three rows of 65 (levels across a 64-index boundary), the same with
the buffer one byte short (a malformed row, reported and bounded), and 257
rows of 64 (two blocks, a ragged last wave).

CASES is imported as data by tests/test_jpeg_decode_host.py.  uint64 arrays
travel as their int64 bit patterns: torch moves bytes.
"""
import ctypes

import numpy as np
import pytest
import torch

import fences
import held_stream
import helpers
import test_image_abi_fences_gpu as image_table
import test_jpeg_abi_gpu as codec_table

pytestmark = pytest.mark.gpu

OK = 0
LEAD = 3
Case, Spec = image_table.Case, image_table.Spec

CASES = []


def case(entry, name):
  def deco(make):
    CASES.append(Case(entry, name, make))
    return make
  return deco


def _strings(array):
  return [b.decode('ascii') for b in array.tolist()]


def _pack(streams):
  bits = np.frombuffer(('1' * LEAD + ''.join(streams)).encode('ascii'),
                       dtype=np.uint8) - ord('0')
  offsets = LEAD + np.concatenate(
      [[0], np.cumsum([len(x) for x in streams])]).astype(np.int64)
  return np.packbits(bits), offsets


def rows_of_65():
  rows = codec_table.fixture_rows()
  packed, offsets = _pack(rows['streams'])
  inputs = {'packed': packed, 'offsets': offsets}
  inputs.update({k: rows[k] for k in ('ac_code', 'ac_len', 'dc_code',
                                      'dc_len')})
  return inputs, rows['levels']


def rows_of_b257():
  from utils import jpeg
  g = helpers.load('jpeg')
  tables = [dict(zip(_strings(g['table_%s_symbols_b257' % kind]),
                     _strings(g['table_%s_codes_b257' % kind])))
            for kind in ('ac', 'dc')]
  ac_code, ac_len = jpeg.table_arrays(tables[0], jpeg._AC_BYTE, 256)
  dc_code, dc_len = jpeg.table_arrays(tables[1], jpeg._DC_CATEGORY, 16)
  packed, offsets = _pack(_strings(g['streams_b257']))
  return ({'packed': packed, 'offsets': offsets,
           'ac_code': ac_code.view(np.int64), 'ac_len': ac_len,
           'dc_code': dc_code.view(np.int64), 'dc_len': dc_len},
          g['levels_b257'].astype(np.int32))


def _unpack_case(rows, missing_bytes):
  def make(lib):
    inputs, levels = rows()
    d, s = levels.shape
    packed_bytes = len(inputs['packed']) - missing_bytes
    inputs['packed'] = np.ascontiguousarray(inputs['packed'][:packed_bytes])
    # the held-stream runner tells staged input from poison by its first word
    assert not (inputs['packed'][:4] == fences.POISON_BYTE).all()
    ws = lib.vtc_jpeg_unpack_workspace_bytes()
    assert ws == 7424

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_jpeg_unpack(
          p['packed'], packed_bytes, p['offsets'], d, s, p['ac_code'],
          p['ac_len'], p['dc_code'], p['dc_len'], p['levels'], p['status'],
          ws_ptr, ws_bytes, stream)

    def truth(res, inputs):
      lost = np.flatnonzero(inputs['offsets'][1:] > 8 * packed_bytes)
      assert len(lost) == (1 if missing_bytes else 0)
      kept = d - len(lost)
      assert np.array_equal(res['levels'][:kept], levels[:kept])
      assert res['status'].tolist() == (
          [len(lost), kept + 1, 0] if missing_bytes else [0, 0, 0])
      assert ((res['levels'][kept:] == 0) |
              (res['levels'][kept:] == levels[kept:])).all()

    return Spec(inputs, {'levels': ((d, s), np.int32),
                         'status': ((3,), np.int64)}, call, truth, ws)
  return make


case('vtc_jpeg_unpack', 'd3-s65')(_unpack_case(rows_of_65, 0))
case('vtc_jpeg_unpack', 'short-d3-s65')(_unpack_case(rows_of_65, 1))
case('vtc_jpeg_unpack', 'd257-s64')(_unpack_case(rows_of_b257, 0))

IDS = [c.id for c in CASES]


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_fenced(device, c):
  image_table.run_case(device, c)


# --------------------------------------------------------- skewed pointers
SKEWS = {'offsets': 8, 'ac_code': 8, 'dc_code': 8, 'ac_len': 3, 'dc_len': 3,
         'levels': 4, 'status': 8}


@pytest.mark.parametrize('packed_skew', [1, 2, 3])
@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_skewed(device, c, packed_skew):
  import vtc_hip
  lib = vtc_hip.load_library()
  spec = c.make(lib)
  stream = vtc_hip.current_stream(device)
  want, _ = codec_table._plain(device, lib, spec, stream)
  spec.truth({k: v.cpu().numpy() for k, v in want.items()}, spec.inputs)

  t, f = {}, {}
  for k, v in spec.inputs.items():
    skew = packed_skew if k == 'packed' else SKEWS[k]
    t[k], f[k] = fences.fenced_copy(v, device, skew=skew)
    assert t[k].data_ptr() % 16 == skew
  for k, (shape, dtype) in spec.outputs.items():
    t[k], f[k] = fences.fenced(shape, codec_table._torch_dtype(dtype), device,
                               skew=SKEWS[k])
    assert t[k].data_ptr() % 16 == SKEWS[k]
  ws, f['workspace'] = fences.fenced_workspace(spec.ws_bytes, device)
  pointers = {k: ctypes.c_void_p(v.data_ptr()) for k, v in t.items()}
  rc = spec.call(lib, pointers, ctypes.c_void_p(ws.data_ptr()), spec.ws_bytes,
                 stream)
  torch.cuda.synchronize(device)
  assert rc == OK, '%s skewed: %s' % (c.id, lib.vtc_last_error())
  for k, fence in f.items():
    fence.assert_intact('%s (packed + %d): %s' % (c.id, packed_skew, k))
  for k, v in spec.inputs.items():
    assert np.array_equal(t[k].cpu().numpy(), v), k
  for k, v in want.items():
    assert torch.equal(t[k], v), (
        '%s (packed + %d): %s differs from the plain call in %d elements'
        % (c.id, packed_skew, k, int((t[k] != v).sum())))


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
  print('jpeg_decode_abi_delay %s' % h.describe())
  return h


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_held_side_stream(device, hold, c):
  codec_table.test_held_side_stream(device, hold, c)
