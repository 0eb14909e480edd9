"""The two writing entry points of include/vtc_index_code.h, three ways
(modelled on tests/test_vq_abi_gpu.py, with the same runners as they are):

  fenced   tests/test_image_abi_fences_gpu.run_case: a plain call, then inputs
           and outputs inside [guard | payload | guard] arenas
           (tests/fences.py), outputs 0xFF-filled, and once more with every
           pointer at its bare element alignment
  skewed   `packed` 1, 2 and 3 bytes past a 16-byte boundary, `len` 1 byte,
           `indices` and `row_bits` 4 bytes, `code`, `offsets`, `column_bits`
           and `status` 8 bytes
  held     on a side stream behind a delay (tests/held_stream.py), every
           payload poisoned until the stream uploads the inputs, canaries on
           the null stream before and after the call; bitwise the
           default-stream result

Two shapes of tests/index_code_data.py: 257 x 42 with kmax = 1024 (one row per
wave step, the experiment's 41 + 1 columns, the 1 .. 64-bit table in column 0)
and 65 x 1 with kmax = 4096 (64 rows per step and one more).  Neither call
takes a workspace.  The truth is the restatement, computed here.
"""
import ctypes

import numpy as np
import pytest
import torch

import fences
import held_stream
import index_code_data as data
import test_image_abi_fences_gpu as image_table
import test_jpeg_abi_gpu as codec_table

pytestmark = pytest.mark.gpu

OK = 0
Case, Spec = image_table.Case, image_table.Spec
SHAPES = [(257, 42, 1024), (65, 1, 4096)]
LEAD = 3

CASES = []


def _inputs(shape):
  from utils import index_coding
  tables, _ = data.case_tables(*shape)
  host = data.case_indices(*shape)
  assert host[0, 0] != -1            # the first word is no poison pattern
  code, length = index_coding.index_table_arrays(tables, shape[2])
  return tables, host, code.view(np.int64), length


def _bits_case(shape):
  b, m, kmax = shape

  def make(lib):
    tables, host, _, length = _inputs(shape)

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_index_code_bits(p['indices'], b, m, p['len'], kmax,
                                     p['row_bits'], p['column_bits'],
                                     p['status'], stream)

    def truth(res, inputs):
      assert np.array_equal(res['row_bits'], data.row_bits(host, tables))
      assert np.array_equal(res['column_bits'],
                            data.column_bits(host, tables))
      assert res['status'].tolist() == [0, 0, 0]

    return Spec({'indices': host, 'len': length},
                {'row_bits': ((b,), np.int32), 'column_bits': ((m,), np.int64),
                 'status': ((3,), np.int64)}, call, truth, 0)
  return make


def _pack_case(shape, missing_bytes):
  b, m, kmax = shape

  def make(lib):
    tables, host, code, length = _inputs(shape)
    offsets = data.layout(data.row_bits(host, tables), LEAD, data.gaps(b))
    nbytes = -(-int(offsets[-1]) // 8) - missing_bytes
    assert nbytes > 8

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_index_code_pack(p['indices'], b, m, p['code'], p['len'],
                                     kmax, p['offsets'], p['packed'], nbytes,
                                     p['status'], stream)

    def truth(res, inputs):
      want, cut = data.image(host, tables, offsets, nbytes)
      assert (cut > 0) == (missing_bytes > 0)
      assert np.array_equal(res['packed'], want)
      assert res['status'].tolist() == [0, 0, cut]

    return Spec({'indices': host, 'code': code, 'len': length,
                 'offsets': offsets},
                {'packed': ((nbytes,), np.uint8), 'status': ((3,), np.int64)},
                call, truth, 0)
  return make


for _shape in SHAPES:
  _name = '%dx%d' % _shape[:2]
  CASES.append(Case('vtc_index_code_bits', _name, _bits_case(_shape)))
  CASES.append(Case('vtc_index_code_pack', _name + '-exact',
                    _pack_case(_shape, 0)))
  CASES.append(Case('vtc_index_code_pack', _name + '-short',
                    _pack_case(_shape, 2)))

IDS = [c.id for c in CASES]


def test_every_writing_entry_point_has_a_row():
  import vtc_hip
  writing = {name for name in vtc_hip.INDEX_CODE_SIGNATURES
             if not name.endswith(('_workspace_bytes', '_abi_version'))}
  assert writing == {c.entry for c in CASES} and len(writing) == 2


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_fenced(device, c):
  image_table.run_case(device, c)


# --------------------------------------------------------- skewed pointers
SKEWED = [(c, skew) for c in CASES for skew in (1, 2, 3)]


@pytest.mark.parametrize('c,byte_skew', SKEWED,
                         ids=['%s+%d' % (c.id, skew) for c, skew in SKEWED])
def test_skewed(device, c, byte_skew):
  """Every pointer at its element alignment and no more; `packed` at each of
  the three odd byte positions of a word."""
  import vtc_hip
  lib = vtc_hip.load_library()
  spec = c.make(lib)
  stream = vtc_hip.current_stream(device)
  want, _ = codec_table._plain(device, lib, spec, stream)
  spec.truth({k: v.cpu().numpy() for k, v in want.items()}, spec.inputs)

  t, f = {}, {}
  for k, v in spec.inputs.items():
    skew = v.dtype.itemsize          # indices 4, code and offsets 8, len 1
    t[k], f[k] = fences.fenced_copy(v, device, skew=skew)
    assert t[k].data_ptr() % 16 == skew
  for k, (shape, dtype) in spec.outputs.items():
    skew = byte_skew if k == 'packed' else np.dtype(dtype).itemsize
    t[k], f[k] = fences.fenced(shape, codec_table._torch_dtype(dtype), device,
                               skew=skew)
    assert t[k].data_ptr() % 16 == skew
  pointers = {k: ctypes.c_void_p(v.data_ptr()) for k, v in t.items()}
  rc = spec.call(lib, pointers, ctypes.c_void_p(0), 0, stream)
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
  print('index_code_abi_delay %s' % h.describe())
  return h


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_held_side_stream(device, hold, c):
  codec_table.test_held_side_stream(device, hold, c)
