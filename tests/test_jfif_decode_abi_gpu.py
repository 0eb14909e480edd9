"""Every writing entry point of include/ext/vtc_jfif_decode.h through raw
ctypes, on the pattern of tests/test_jfif_abi_gpu.py with the same runners as
they are:

  fenced   tests/test_image_abi_fences_gpu.run_case: a plain call, then
           inputs, outputs and workspace inside [guard | payload | guard]
           arenas (tests/fences.py), outputs and workspace 0xFF-filled, the
           workspace of EXACTLY the queried size, and once more with every
           pointer at its bare element alignment; one byte less workspace
           answers VTC_ERR_WORKSPACE and touches nothing
  skewed1  tests/test_jfif_abi_gpu.test_skewed_by_one_element: every uint8
           array one byte past a 16-byte boundary (the segment, whose words
           the unpack kernel loads aligned, among them), every other array one
           element past one
  held     on a side stream behind a delay (tests/held_stream.py)

vtc_jfif_dc_accumulate updates levels in place, which the runners' "inputs
stay as they were" does not allow: its rows copy the DIFF levels into the
output with hipMemcpyAsync on the call's stream and accumulate there.

The truth is tests/jfif_decode_data.py, exact equality throughout.  uint16
arrays travel as their int16 bit patterns: torch moves bytes."""
import ctypes

import numpy as np
import pytest
import torch

import fences
import jfif_decode_data as dd
import test_image_abi_fences_gpu as image_table
import test_jfif_abi_gpu as jfif_table
import test_jpeg_abi_gpu as codec_table

pytestmark = pytest.mark.gpu

Case, Spec = image_table.Case, image_table.Spec
CASES = []


def case(entry, name):
  def deco(make):
    CASES.append(Case(entry, name, make))
    return make
  return deco


_runtime = []


def _hip():
  """The HIP runtime torch has loaded, for hipMemcpyAsync."""
  if not _runtime:
    path = None
    with open('/proc/self/maps') as maps:
      for line in maps:
        if 'libamdhip64' in line:
          path = line.split()[-1]
          break
    assert path, 'torch has not loaded the HIP runtime'
    lib = ctypes.CDLL(path)
    lib.hipMemcpyAsync.restype = ctypes.c_int
    lib.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_size_t, ctypes.c_int,
                                   ctypes.c_void_p]
    _runtime.append(lib)
  return _runtime[0]


DEVICE_TO_DEVICE = 3


def _unstuff_case(n, short):
  def make(lib):
    rs = np.random.RandomState(n)
    raw = rs.randint(0, 255, size=n).astype(np.uint8)
    raw[rs.rand(n) < 0.15] = 0xFF
    data = bytearray(dd.truth.stuff(raw.tobytes())[:n - 3] + b'\x02\xff\xd9')
    if data[n - 4] == 0xFF:     # its 0x00 was cut off
      data[n - 4] = 0x01
    # a pair across the first tile boundary, neutral bytes around it
    data[2044:2052] = b'\x01\x01\x01\xff\x00\x01\x01\x01'
    if data[2043] == 0xFF:
      data[2043] = 0x01
    data[0:2] = b'\x12\x13'     # the held-stream canary reads these bytes
    data = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    assert data[2047] == 0xFF and data[2048] == 0x00
    want, marker_at = dd.unstuff(data.tobytes())
    assert marker_at == n - 2 and len(want) < marker_at - 400
    capacity = len(want) - short
    ws = lib.vtc_jfif_unstuff_bytes_workspace_bytes(n)
    tiles = -(-n // 2048)
    assert ws == 2 * 256 * -(-8 * tiles // 256) + 256

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_jfif_unstuff_bytes(p['in'], n, p['out'], capacity,
                                        p['out_len'], p['status'], ws_ptr,
                                        ws_bytes, stream)

    def check(res, inputs):
      assert res['out'].tobytes() == want[:capacity]
      assert res['out_len'].tolist() == [len(want), marker_at]
      assert res['status'].tolist() == [short]

    return Spec({'in': data}, {'out': ((capacity,), np.uint8),
                               'out_len': ((2,), np.int64),
                               'status': ((1,), np.int32)}, call, check, ws)
  return make


def _unpack_case(d, density):
  def make(lib):
    rs = np.random.RandomState(d)
    levels = (rs.randint(-300, 301, size=(d, 64)) *
              (rs.rand(d, 64) < density)).astype(np.int32)
    levels[:, 0] = rs.randint(-700, 701, size=d)
    levels[d - 1, 63] = -1                    # no end of block
    raw, tables, offsets = dd.pack_host(levels)
    arrays = dd.table_arrays(tables)
    seg = np.frombuffer(raw, dtype=np.uint8).copy()
    n = len(seg)
    ws = lib.vtc_jfif_unpack_workspace_bytes(n)
    groups = -(-n // dd.GROUP_BYTES)
    assert ws > 0 and (groups > 1) == (d > 100)
    slots = np.zeros(3, dtype=np.uint8)       # three positions, one table

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_jfif_unpack(p['seg'], n, p['slot_dc'], p['slot_ac'], 3,
                                 p['ac_code'], p['ac_len'], p['dc_code'],
                                 p['dc_len'], p['levels'], d, p['status'],
                                 ws_ptr, ws_bytes, stream)

    def check(res, inputs):
      assert np.array_equal(res['levels'], dd.diffs_of(levels))
      assert res['status'].tolist()[:3] == [0, d, int(offsets[-1])]
      assert res['status'][3] >= 1

    return Spec({'seg': seg, 'slot_dc': slots, 'slot_ac': slots.copy(),
                 'ac_code': arrays['ac_code'].view(np.int16),
                 'ac_len': arrays['ac_len'],
                 'dc_code': arrays['dc_code'].view(np.int16),
                 'dc_len': arrays['dc_len']},
                {'levels': ((d, 64), np.int32), 'status': ((4,), np.int64)},
                call, check, ws)
  return make


def _dc_case(d):
  def make(lib):
    rs = np.random.RandomState(d)
    diff = rs.randint(-2047, 2048, size=(d, 64)).astype(np.int32)
    diff[0, 0] = 77       # the held-stream canary reads these four bytes
    order = rs.permutation(d).astype(np.int32)
    if d > 2:
      order[1] = d        # adds nothing, writes nothing
    start = (rs.rand(d) < 0.05).astype(np.uint8)
    start[0] = 1
    want = dd.dc_accumulate(diff, order, start)
    ws = lib.vtc_jfif_dc_accumulate_workspace_bytes(d)
    assert ws == 2 * 256 * -(-4 * -(-d // 256) // 256)

    def call(lib, p, ws_ptr, ws_bytes, stream):
      if ws_bytes >= ws:    # a call that is refused must find levels untouched
        rc = _hip().hipMemcpyAsync(p['levels'], p['diff'], diff.nbytes,
                                   DEVICE_TO_DEVICE, stream)
        assert rc == 0
      return lib.vtc_jfif_dc_accumulate(p['levels'], d, p['order'],
                                        p['start'], ws_ptr, ws_bytes, stream)

    def check(res, inputs):
      assert np.array_equal(res['levels'], want)

    return Spec({'diff': diff, 'order': order, 'start': start},
                {'levels': ((d, 64), np.int32)}, call, check, ws)
  return make


case('vtc_jfif_unstuff_bytes', 'n4097-exact')(_unstuff_case(4097, 0))
case('vtc_jfif_unstuff_bytes', 'n4097-one-short')(_unstuff_case(4097, 1))
case('vtc_jfif_unpack', 'd5-one-group')(_unpack_case(5, 0.3))
case('vtc_jfif_unpack', 'd1200-two-groups')(_unpack_case(1200, 0.3))
case('vtc_jfif_dc_accumulate', 'd1')(_dc_case(1))
case('vtc_jfif_dc_accumulate', 'd300')(_dc_case(300))

IDS = [c.id for c in CASES]


def test_every_writing_entry_point_has_a_row():
  import vtc_hip
  writing = {name for name in vtc_hip.JFIF_DECODE_BINDINGS
             if not name.endswith(('_abi_version', '_workspace_bytes'))}
  assert writing == {c.entry for c in CASES} and len(writing) == 3


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_fenced(device, c):
  image_table.run_case(device, c)


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_skewed_by_one_element(device, c):
  jfif_table.test_skewed_by_one_element(device, c)


def test_null_pointers_and_bad_sizes_touch_nothing(device):
  """The refusals come before device work: the outputs keep their poison."""
  import vtc_hip
  lib = vtc_hip.load_library()
  stream = vtc_hip.current_stream(device)
  out, fence = fences.fenced((64,), torch.uint8, device)
  length, length_fence = fences.fenced((2,), torch.int64, device)
  status, status_fence = fences.fenced((4,), torch.int64, device)
  levels, levels_fence = fences.fenced((2, 64), torch.int32, device)
  raw = torch.zeros(64, dtype=torch.uint8, device=device)
  big = torch.zeros(1 << 16, dtype=torch.uint8, device=device)
  p = lambda x: ctypes.c_void_p(x.data_ptr())
  null = ctypes.c_void_p(0)
  assert lib.vtc_jfif_unstuff_bytes(null, 64, p(out), 64, p(length),
                                    p(status), p(big), 1 << 16, stream) == 1
  assert lib.vtc_jfif_unstuff_bytes(p(raw), 64, p(out), 64, p(length),
                                    p(status), null, 0, stream) == 3
  assert lib.vtc_jfif_unstuff_bytes(p(raw), -1, p(out), 64, p(length),
                                    p(status), p(big), 1 << 16, stream) == 1
  unpack = [p(raw), 64, p(raw), p(raw), 1, p(raw), p(raw), p(raw), p(raw),
            p(levels), 2, p(status), p(big), 1 << 16, stream]
  for i, bad in ((0, null), (1, 0), (4, 0), (4, 11), (9, null), (10, 0),
                 (11, null)):
    assert lib.vtc_jfif_unpack(*(unpack[:i] + [bad] + unpack[i + 1:])) == 1
  assert lib.vtc_jfif_unpack(*(unpack[:13] + [255] + unpack[14:])) == 3
  dc = [p(levels), 2, p(raw), p(raw), p(big), 1 << 16, stream]
  for i, bad in ((0, null), (1, 0), (2, null), (3, null)):
    assert lib.vtc_jfif_dc_accumulate(*(dc[:i] + [bad] + dc[i + 1:])) == 1
  assert lib.vtc_jfif_dc_accumulate(*(dc[:5] + [255] + dc[6:])) == 3
  torch.cuda.synchronize(device)
  for name, fe in (('out', fence), ('out_len', length_fence),
                   ('status', status_fence), ('levels', levels_fence)):
    fe.assert_intact(name)
    fe.assert_untouched(name)


def test_workspace_queries(device):
  """What the queries answer is what the calls ask for (the fenced rows run
  each call on exactly that, and on one byte less), it grows by whole
  workgroups and tiles, and sizes outside a call's range answer 0."""
  import vtc_hip
  lib = vtc_hip.load_library()
  one = lib.vtc_jfif_unpack_workspace_bytes(1)
  assert one == lib.vtc_jfif_unpack_workspace_bytes(dd.GROUP_BYTES)
  two = lib.vtc_jfif_unpack_workspace_bytes(dd.GROUP_BYTES + 1)
  # per workgroup: 256 subsequences of two words, and seven arrays' entries
  assert two - one == 2 * 256 * 4 and one % 256 == 0
  assert lib.vtc_jfif_unpack_workspace_bytes(0) == 0
  assert lib.vtc_jfif_unpack_workspace_bytes(1 << 31) == 0
  assert lib.vtc_jfif_unstuff_bytes_workspace_bytes(2048) == 3 * 256
  assert lib.vtc_jfif_unstuff_bytes_workspace_bytes(2049) == 3 * 256
  assert lib.vtc_jfif_unstuff_bytes_workspace_bytes(2048 * 32 + 1) == 5 * 256
  assert lib.vtc_jfif_dc_accumulate_workspace_bytes(256 * 64) == 2 * 256
  assert lib.vtc_jfif_dc_accumulate_workspace_bytes(256 * 64 + 1) == 4 * 256


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
  print('jfif_decode_abi_delay %s' % h.describe())
  return h


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_held_side_stream(device, hold, c):
  codec_table.test_held_side_stream(device, hold, c)
