"""vtc_ssim, the writing entry point of include/vtc_quality.h, three ways
(modelled on tests/test_jpeg_decode_abi_gpu.py, with the same runners):

  fenced   tests/test_image_abi_fences_gpu.run_case as it is: a plain call,
           then inputs, outputs and workspace inside [guard | payload | guard]
           arenas (tests/fences.py), outputs and workspace 0xFF-filled, the
           workspace of EXACTLY the queried size, every output element
           written; one byte less workspace must answer VTC_ERR_WORKSPACE and
           touch nothing
  skewed   float32 images 4, 8 and 12 bytes past a 16-byte boundary, float64
           images 8; data_range, mean_out and map_out 8
  held     on a side stream behind a delay (tests/held_stream.py), every
           payload poisoned until the stream uploads the inputs, canaries on
           the null stream before and after the call; bitwise the
           default-stream result

The cases: three images of 12 x 17 with three ranges, and one image of 17 x 33
(one 16 x 32 tile plus one sample in each axis: four blocks, three of them
nearly empty), float32 and float64, with the map and with map_out = NULL.
The truth is tests/ssim_oracle.py at the 1e-9 of tests/test_ssim_gpu.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import fences
import held_stream
import ssim_oracle
import test_image_abi_fences_gpu as image_table
import test_jpeg_abi_gpu as codec_table

pytestmark = pytest.mark.gpu

OK = 0
F32, F64 = 0, 2
BOUND = 1e-9
Case, Spec = image_table.Case, image_table.Spec

CASES = []


def case(entry, name):
  def deco(make):
    CASES.append(Case(entry, name, make))
    return make
  return deco


def _ssim_case(count, h, w, dtype, with_map):
  def make(lib):
    rs = np.random.RandomState(100 * count + h + w + dtype)
    np_dtype = np.float32 if dtype == F32 else np.float64
    ranges = np.array([1.0, 255.0, 0.75][:count])
    x = (rs.rand(count, h, w) * ranges[:, None, None]).astype(np_dtype)
    y = np.clip(x + 0.1 * ranges[:, None, None] * rs.randn(count, h, w),
                0, None).astype(np_dtype)
    assert all(max(x[i].max(), y[i].max()) <= 2 * ranges[i]
               for i in range(count))
    ws = lib.vtc_ssim_workspace_bytes(count, h, w)
    assert ws == -(-8 * count * -(-h // 16) * -(-w // 32) // 256) * 256

    def call(lib, p, ws_ptr, ws_bytes, stream):
      return lib.vtc_ssim(p['x'], p['y'], dtype, p['data_range'], p['mean'],
                          p['map'] if with_map else None, count, h, w, ws_ptr,
                          ws_bytes, stream)

    def truth(res, inputs):
      for i in range(count):
        mean, smap = ssim_oracle.ssim(inputs['x'][i], inputs['y'][i],
                                      ranges[i])
        assert abs(res['mean'][i] - mean) <= BOUND
        if with_map:
          assert np.abs(res['map'][i] - smap).max() <= BOUND

    outputs = {'mean': ((count,), np.float64)}
    if with_map:
      outputs['map'] = ((count, h, w), np.float64)
    return Spec({'x': x, 'y': y, 'data_range': ranges}, outputs, call, truth,
                ws)
  return make


for _count, _h, _w in ((3, 12, 17), (1, 17, 33)):
  for _dtype, _name in ((F32, 'f32'), (F64, 'f64')):
    for _with_map in (True, False):
      case('vtc_ssim', '%dx%dx%d-%s-%s' % (
          _count, _h, _w, _name, 'map' if _with_map else 'nomap'))(
              _ssim_case(_count, _h, _w, _dtype, _with_map))

IDS = [c.id for c in CASES]


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_fenced(device, c):
  image_table.run_case(device, c)


# --------------------------------------------------------- skewed pointers
# float64 needs 8-byte alignment: 8 is its only skew
SKEWED = [(c, skew) for c in CASES
          for skew in ((4, 8, 12) if '-f32-' in c.id else (8,))]


@pytest.mark.parametrize('c,image_skew', SKEWED,
                         ids=['%s+%d' % (c.id, skew) for c, skew in SKEWED])
def test_skewed(device, c, image_skew):
  import vtc_hip
  lib = vtc_hip.load_library()
  spec = c.make(lib)
  stream = vtc_hip.current_stream(device)
  want, _ = codec_table._plain(device, lib, spec, stream)
  spec.truth({k: v.cpu().numpy() for k, v in want.items()}, spec.inputs)

  t, f = {}, {}
  for k, v in spec.inputs.items():
    skew = image_skew if k in ('x', 'y') else 8
    t[k], f[k] = fences.fenced_copy(v, device, skew=skew)
    assert t[k].data_ptr() % 16 == skew
  for k, (shape, dtype) in spec.outputs.items():
    t[k], f[k] = fences.fenced(shape, codec_table._torch_dtype(dtype), device,
                               skew=8)
    assert t[k].data_ptr() % 16 == 8
  ws, f['workspace'] = fences.fenced_workspace(spec.ws_bytes, device)
  pointers = {k: ctypes.c_void_p(v.data_ptr()) for k, v in t.items()}
  rc = spec.call(lib, pointers, ctypes.c_void_p(ws.data_ptr()), spec.ws_bytes,
                 stream)
  torch.cuda.synchronize(device)
  assert rc == OK, '%s skewed: %s' % (c.id, lib.vtc_last_error())
  for k, fence in f.items():
    fence.assert_intact('%s (images + %d): %s' % (c.id, image_skew, k))
  for k, v in spec.inputs.items():
    assert np.array_equal(t[k].cpu().numpy(), v), k
  for k, v in want.items():
    f[k].assert_written('%s (images + %d): %s' % (c.id, image_skew, k))
    assert torch.equal(t[k], v), (
        '%s (images + %d): %s differs from the plain call in %d elements'
        % (c.id, image_skew, k, int((t[k] != v).sum())))


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
  print('ssim_abi_delay %s' % h.describe())
  return h


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_held_side_stream(device, hold, c):
  codec_table.test_held_side_stream(device, hold, c)
