"""vtc_color_transform, vtc_plane_downsample and vtc_plane_upsample, the
writing entry points of include/ext/vtc_color.h, three ways (modelled on
tests/test_index_ans_split_abi_gpu.py, with the same runners as they are):

  fenced   tests/test_image_abi_fences_gpu.run_case: a plain call, then inputs
           and outputs inside [guard | payload | guard] arenas
           (tests/fences.py), outputs 0xFF-filled and every element written,
           and once more with every pointer at its bare element alignment.
           None of the three calls takes a workspace.
  skewed   every device pointer 4 bytes past a 16-byte boundary, bitwise the
           aligned result: the transform then leaves its 16-byte path for the
           element-by-element one
  held     on a side stream behind a delay (tests/held_stream.py), every
           payload poisoned until the stream uploads the inputs, canaries on
           the null stream before and after the call; bitwise the
           default-stream result

(2, 33, 65) stacks: the transform from channel-last to planar, both resamplers
at factors (2, 2), so 33 x 65 against 17 x 33 with a ragged last row and
column.  matrix, pre and post are host arrays that the call closure owns.  The
truth is the restatement of tests/color_data.py, bit for bit.
"""
import ctypes

import numpy as np
import pytest
import torch

import color_data as truth
import fences
import held_stream
import test_image_abi_fences_gpu as image_table
import test_jpeg_abi_gpu as codec_table

pytestmark = pytest.mark.gpu

OK = 0
Case, Spec = image_table.Case, image_table.Spec
COUNT, H, W = 2, 33, 65
FV = FH = 2
HS, WS = -(-H // FV), -(-W // FH)

CASES = []


def _doubles(values):
  values = np.asarray(values, dtype=np.float64).reshape(-1).tolist()
  return (ctypes.c_double * len(values))(*values)


def _transform_case(matrix, pre, post, clamp):
  def make(lib):
    rs = np.random.RandomState(65)
    host = (rs.rand(COUNT, H, W, 3) * 400. - 70.).astype(np.float32)
    # host memory, alive as long as the closure
    m, a, b = _doubles(matrix), _doubles(pre), _doubles(post)

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_color_transform(
          p['in'], truth.HWC, p['out'], truth.CHW, COUNT, H, W,
          ctypes.cast(m, ctypes.c_void_p), ctypes.cast(a, ctypes.c_void_p),
          ctypes.cast(b, ctypes.c_void_p), 0 if clamp is None else 1,
          *(clamp or (0., 0.)), stream)

    def check(res, inputs):
      want = truth.color_transform(inputs['in'], matrix, pre, post, clamp,
                                   truth.HWC, truth.CHW)
      assert truth.same_bits(res['out'], want)

    return Spec({'in': host}, {'out': ((COUNT, 3, H, W), np.float32)}, call,
                check, 0)
  return make


def _downsample_case(lib):
  host = truth.plane_stack(COUNT, H, W, seed=2)

  def call(lib, p, ws_ptr, ws_bytes, stream):
    return lib.vtc_plane_downsample(p['in'], p['out'], COUNT, H, W, FV, FH,
                                    stream)

  def check(res, inputs):
    assert truth.same_bits(res['out'], truth.downsample(inputs['in'], FV, FH))

  return Spec({'in': host}, {'out': ((COUNT, HS, WS), np.float32)}, call,
              check, 0)


def _upsample_case(mode):
  def make(lib):
    host = truth.plane_stack(COUNT, HS, WS, seed=3)

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_plane_upsample(p['in'], p['out'], COUNT, HS, WS, H, W,
                                    FV, FH, mode, stream)

    def check(res, inputs):
      assert truth.same_bits(
          res['out'], truth.upsample(inputs['in'], FV, FH, (H, W), mode))

    return Spec({'in': host}, {'out': ((COUNT, H, W), np.float32)}, call,
                check, 0)
  return make


CASES.append(Case('vtc_color_transform', 'forward-hwc-chw', _transform_case(
    truth.FORWARD, (0., 0., 0.), (0., 128., 128.), None)))
CASES.append(Case('vtc_color_transform', 'dense-clamped-hwc-chw',
                  _transform_case(truth.DENSE, truth.DENSE_PRE,
                                  truth.DENSE_POST, (-50., 300.))))
CASES.append(Case('vtc_plane_downsample', '2x2', _downsample_case))
CASES.append(Case('vtc_plane_upsample', 'replicate-2x2',
                  _upsample_case(truth.REPLICATE)))
CASES.append(Case('vtc_plane_upsample', 'triangle-2x2',
                  _upsample_case(truth.TRIANGLE)))

IDS = [c.id for c in CASES]


def test_every_writing_entry_point_has_a_row():
  import vtc_hip
  writing = {name for name in vtc_hip.COLOR_BINDINGS
             if not name.endswith('_abi_version')}
  assert writing == {c.entry for c in CASES} and len(writing) == 3


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_fenced(device, c):
  image_table.run_case(device, c)


# --------------------------------------------------------- skewed pointers
@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_skewed(device, c):
  """Every device pointer 4 bytes past a 16-byte boundary."""
  import vtc_hip
  lib = vtc_hip.load_library()
  spec = c.make(lib)
  stream = vtc_hip.current_stream(device)
  want, _ = codec_table._plain(device, lib, spec, stream)
  spec.truth({k: v.cpu().numpy() for k, v in want.items()}, spec.inputs)

  t, f = {}, {}
  for k, v in spec.inputs.items():
    t[k], f[k] = fences.fenced_copy(v, device, skew=4)
  for k, (shape, dtype) in spec.outputs.items():
    t[k], f[k] = fences.fenced(shape, codec_table._torch_dtype(dtype), device,
                               skew=4)
  for k, v in t.items():
    assert v.data_ptr() % 16 == 4, k
  pointers = {k: ctypes.c_void_p(v.data_ptr()) for k, v in t.items()}
  rc = spec.call(lib, pointers, ctypes.c_void_p(0), 0, stream)
  torch.cuda.synchronize(device)
  assert rc == OK, '%s skewed: %s' % (c.id, lib.vtc_last_error())
  for k, fence in f.items():
    fence.assert_intact('%s (+4): %s' % (c.id, k))
  for k, v in spec.inputs.items():
    assert np.array_equal(t[k].cpu().numpy(), v), k
  for k, v in want.items():
    f[k].assert_written('%s (+4): %s' % (c.id, k))
    assert torch.equal(t[k], v), (
        '%s (+4): %s differs from the plain call in %d elements'
        % (c.id, k, int((t[k] != v).sum())))


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
  print('color_abi_delay %s' % h.describe())
  return h


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_held_side_stream(device, hold, c):
  codec_table.test_held_side_stream(device, hold, c)
