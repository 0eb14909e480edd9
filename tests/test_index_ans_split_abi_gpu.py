"""vtc_index_ans_split_sizes, vtc_index_ans_split_pack and
vtc_index_ans_split_unpack, the writing entry points of
include/ext/vtc_index_ans_split.h, three ways (modelled on
tests/test_index_ans_abi_gpu.py, with the same runners as they are):

  fenced   tests/test_image_abi_fences_gpu.run_case: a plain call, then inputs,
           outputs and workspace inside [guard | payload | guard] arenas
           (tests/fences.py), outputs and workspace 0xFF-filled, the workspace
           of EXACTLY the queried size, and once more with every pointer at its
           bare element alignment; one byte less workspace must answer
           VTC_ERR_WORKSPACE and touch nothing
  skewed   `packed` 1, 2 and 3 bytes past a 16-byte boundary, `freq_hi` and
           `freq_lo` 2 bytes, `indices`, `stream_bytes` and `used_bytes` 4
           bytes, `offsets` and `status` 8 bytes, the workspace 256-byte
           aligned
  held     on a side stream behind a delay (tests/held_stream.py), every
           payload poisoned until the stream uploads the inputs, canaries on
           the null stream before and after the call; bitwise the
           default-stream result

Two shapes of tests/index_ans_split_data.py: 300 rows at 100 rows per stream
with kmax = 5000 (three streams, a last, partial block) and 65 rows in one
stream with kmax = 131072 (one symbol into a second step, the widest tables).
The streams lie behind three leading bytes with gaps between them; the truth
is the restatement.  uint16 arrays travel as their int16 bit patterns.
"""
import ctypes

import numpy as np
import pytest
import torch

import fences
import held_stream
import index_ans_split_data as truth
import test_image_abi_fences_gpu as image_table
import test_jpeg_abi_gpu as codec_table

pytestmark = pytest.mark.gpu

OK = 0
Case, Spec = image_table.Case, image_table.Spec
SHAPES = [(300, 5000, 100), (65, 131072, 65)]
LEAD = 3

CASES = []


def _inputs(shape):
  host = truth.case_indices(*shape)
  assert host[0] != -1               # the first word is no poison pattern
  freq_hi, freq_lo = truth.case_tables(*shape)
  streams = truth.case_streams(*shape)
  sizes = np.array([len(s) for s in streams], np.int32)
  offsets = truth.layout(sizes, LEAD, truth.gaps(len(streams)))
  freq = {'freq_hi': freq_hi.view(np.int16), 'freq_lo': freq_lo.view(np.int16)}
  return host, freq, streams, sizes, offsets


def _sizes_case(shape):
  b, kmax, rows = shape

  def make(lib):
    host, freq, _, sizes, _ = _inputs(shape)
    ws = lib.vtc_index_ans_split_workspace_bytes(kmax)
    assert ws > 0

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_index_ans_split_sizes(
          p['indices'], b, p['freq_hi'], p['freq_lo'], kmax, rows,
          p['stream_bytes'], p['status'], ws_ptr, ws_bytes, stream)

    def check(res, inputs):
      assert np.array_equal(res['stream_bytes'], sizes)
      assert res['status'].tolist() == [0, 0, 0]

    return Spec(dict(freq, indices=host),
                {'stream_bytes': ((len(sizes),), np.int32),
                 'status': ((3,), np.int64)}, call, check, ws)
  return make


def _pack_case(shape, missing_bytes):
  b, kmax, rows = shape

  def make(lib):
    host, freq, streams, sizes, offsets = _inputs(shape)
    nbytes = int(offsets[-1]) - missing_bytes
    ws = lib.vtc_index_ans_split_workspace_bytes(kmax)

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_index_ans_split_pack(
          p['indices'], b, p['freq_hi'], p['freq_lo'], kmax, rows,
          p['stream_bytes'], p['offsets'], p['packed'], nbytes, p['status'],
          ws_ptr, ws_bytes, stream)

    def check(res, inputs):
      want, skipped = truth.image(streams, offsets, nbytes)
      assert (skipped > 0) == (missing_bytes > 0)
      assert np.array_equal(res['packed'], want)
      assert res['status'].tolist() == [0, 0, skipped]

    return Spec(dict(freq, indices=host, stream_bytes=sizes, offsets=offsets),
                {'packed': ((nbytes,), np.uint8), 'status': ((3,), np.int64)},
                call, check, ws)
  return make


def _unpack_case(shape):
  b, kmax, rows = shape

  def make(lib):
    host, freq, streams, sizes, offsets = _inputs(shape)
    packed, _ = truth.image(streams, offsets, int(offsets[-1]))
    nbytes = len(packed)
    # the held-stream runner tells staged input from poison by its first word
    assert not (packed[:4] == fences.POISON_BYTE).all()
    ws = lib.vtc_index_ans_split_workspace_bytes(kmax)

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_index_ans_split_unpack(
          p['packed'], nbytes, p['offsets'], b, p['freq_hi'], p['freq_lo'],
          kmax, rows, p['indices'], p['used_bytes'], p['status'], ws_ptr,
          ws_bytes, stream)

    def check(res, inputs):
      assert np.array_equal(res['indices'], host)
      assert np.array_equal(res['used_bytes'], sizes)
      assert res['status'].tolist() == [0, 0, 0]

    return Spec(dict(freq, packed=packed, offsets=offsets),
                {'indices': ((b,), np.int32),
                 'used_bytes': ((len(sizes),), np.int32),
                 'status': ((3,), np.int64)}, call, check, ws)
  return make


for _shape in SHAPES:
  _name = '%d-k%d' % _shape[:2]
  CASES.append(Case('vtc_index_ans_split_sizes', _name, _sizes_case(_shape)))
  CASES.append(Case('vtc_index_ans_split_pack', _name + '-exact',
                    _pack_case(_shape, 0)))
  CASES.append(Case('vtc_index_ans_split_pack', _name + '-short',
                    _pack_case(_shape, 2)))
  CASES.append(Case('vtc_index_ans_split_unpack', _name, _unpack_case(_shape)))

IDS = [c.id for c in CASES]


def test_every_writing_entry_point_has_a_row():
  import vtc_hip
  writing = {name for name in vtc_hip.INDEX_ANS_SPLIT_BINDINGS
             if not name.endswith(('_workspace_bytes', '_abi_version'))}
  assert writing == {c.entry for c in CASES} and len(writing) == 3


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_fenced(device, c):
  image_table.run_case(device, c)


# --------------------------------------------------------- skewed pointers
SKEWED = [(c, skew) for c in CASES for skew in (1, 2, 3)
          if c.entry != 'vtc_index_ans_split_sizes']


@pytest.mark.parametrize('c,byte_skew', SKEWED,
                         ids=['%s+%d' % (c.id, skew) for c, skew in SKEWED])
def test_skewed(device, c, byte_skew):
  """Every pointer at its element alignment and no more; `packed` at each of
  the three odd byte positions of a word; the workspace of exactly the
  queried size."""
  import vtc_hip
  lib = vtc_hip.load_library()
  spec = c.make(lib)
  stream = vtc_hip.current_stream(device)
  want, _ = codec_table._plain(device, lib, spec, stream)
  spec.truth({k: v.cpu().numpy() for k, v in want.items()}, spec.inputs)

  t, f = {}, {}
  for k, v in spec.inputs.items():
    # freq_hi and freq_lo 2, indices and stream_bytes 4, offsets 8
    skew = byte_skew if k == 'packed' else v.dtype.itemsize
    t[k], f[k] = fences.fenced_copy(v, device, skew=skew)
    assert t[k].data_ptr() % 16 == skew
  for k, (shape, dtype) in spec.outputs.items():
    # indices and used_bytes 4, status 8
    skew = byte_skew if k == 'packed' else np.dtype(dtype).itemsize
    t[k], f[k] = fences.fenced(shape, codec_table._torch_dtype(dtype), device,
                               skew=skew)
    assert t[k].data_ptr() % 16 == skew
  ws, f['workspace'] = fences.fenced_workspace(spec.ws_bytes, device)
  assert ws.data_ptr() % 256 == 0
  pointers = {k: ctypes.c_void_p(v.data_ptr()) for k, v in t.items()}
  rc = spec.call(lib, pointers, ctypes.c_void_p(ws.data_ptr()), spec.ws_bytes,
                 stream)
  torch.cuda.synchronize(device)
  assert rc == OK, '%s skewed: %s' % (c.id, lib.vtc_last_error())
  for k, fence in f.items():
    fence.assert_intact('%s (+%d): %s' % (c.id, byte_skew, k))
  for k, v in spec.inputs.items():
    assert np.array_equal(t[k].cpu().numpy(), v), k
  for k, v in want.items():
    assert torch.equal(t[k], v), (
        '%s (+%d): %s differs from the plain call in %d elements'
        % (c.id, byte_skew, k, int((t[k] != v).sum())))


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
  print('index_ans_split_abi_delay %s' % h.describe())
  return h


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_held_side_stream(device, hold, c):
  codec_table.test_held_side_stream(device, hold, c)
