"""The three kernels of include/ext/vtc_color.h against the float64
restatement of tests/color_data.py, bit for bit: the header fixes the order of
every operation, so there is no tolerance.  NaNs compare as a class
(color_data.bits), everything else by its bit pattern.

color_transform runs every case three ways and must give the same bits each
time: as the shape selects its path (16-byte groups of 4 pixels where the
arrays allow it), with the grid capped at one block through
VTC_COLOR_MAX_BLOCKS so that the grid-stride loops turn over, and through the
raw entry point on pointers 4 bytes past a 16-byte boundary, which takes the
element-by-element path.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import color_data as truth
import helpers

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 7), (2, 33, 65), (1, 64, 257)]
PLANES = [(1, 1, 1), (3, 5, 7), (2, 33, 65), (1, 16, 64)]
OUT_SHAPES = [(1, 1), (5, 7), (33, 65), (16, 64)]
LAYOUTS = [('hwc', 'hwc'), ('hwc', 'chw'), ('chw', 'hwc'), ('chw', 'chw')]
CODE = {'hwc': truth.HWC, 'chw': truth.CHW}
O = 128.0
MAPS = {
    'forward': (truth.FORWARD, None, (0., O, O), None),
    'inverse': (truth.INVERSE, (0., O, O), None, None),
    'inverse-clamped': (truth.INVERSE, (0., O, O), None, (0., 255.)),
    'dense': (truth.DENSE, truth.DENSE_PRE, truth.DENSE_POST, None),
}


@pytest.fixture
def one_block():
  """Caps the grid of the colour kernels at one block of 256 threads."""
  def run(fn):
    os.environ['VTC_COLOR_MAX_BLOCKS'] = '1'
    try:
      return fn()
    finally:
      del os.environ['VTC_COLOR_MAX_BLOCKS']
  return run


def _skewed(host, device):
  """`host` on the device, 4 bytes past a 16-byte boundary."""
  arena = torch.empty(host.size + 8, dtype=torch.float32, device=device)
  view = arena[1:1 + host.size].view(host.shape)
  view.copy_(torch.from_numpy(host))
  assert view.data_ptr() % 16 == 4 and view.is_contiguous()
  return view


def _raw_transform(device, host, shape, name, layout, out_layout):
  """The entry point itself, both arrays at bare element alignment."""
  import vtc_hip
  lib = vtc_hip.load_library()
  matrix, pre, post, clamp = MAPS[name]
  doubles = [(ctypes.c_double * len(v))(*v) for v in (
      np.asarray(matrix, dtype=np.float64).reshape(-1).tolist(),
      list(pre or (0., 0., 0.)), list(post or (0., 0., 0.)))]
  count, h, w = shape
  x = _skewed(host, device)
  out = _skewed(np.zeros(host.size, np.float32), device)
  rc = lib.vtc_color_transform(
      vtc_hip.ptr(x), CODE[layout], vtc_hip.ptr(out), CODE[out_layout], count,
      h, w, *[ctypes.cast(d, ctypes.c_void_p) for d in doubles],
      0 if clamp is None else 1, *(clamp or (0., 0.)),
      vtc_hip.current_stream(device))
  assert rc == 0, lib.vtc_last_error()
  torch.cuda.synchronize(device)
  return out.cpu().numpy()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('layouts', LAYOUTS, ids=lambda p: '%s-%s' % p)
@pytest.mark.parametrize('name', sorted(MAPS))
def test_color_transform(device, one_block, name, layouts, shape):
  from utils import color
  layout, out_layout = layouts
  matrix, pre, post, clamp = MAPS[name]
  host = truth.wild_stack(*shape, layout=CODE[layout])
  if host.size >= 48:
    assert np.isnan(host).sum() == 1 and np.isinf(host).sum() == 2
    assert (host[np.isfinite(host)] < 0).any() and (host > 255).any()
  want = truth.color_transform(host, matrix, pre, post, clamp, CODE[layout],
                               CODE[out_layout])
  x = helpers.to_dev(host, device)

  def run():
    return color.color_transform(x, matrix, pre, post, clamp, layout,
                                 out_layout)
  got = run()
  assert got.shape == want.shape and got.dtype == torch.float32
  assert truth.same_bits(got.cpu().numpy(), want)
  assert torch.equal(got.view(torch.int32), run().view(torch.int32))
  assert truth.same_bits(x.cpu().numpy(), host)
  # one block of 256 threads: 64 x 257 pixels are 65 turns of the loop
  capped = one_block(run)
  assert truth.same_bits(capped.cpu().numpy(), want)
  # the element-by-element path
  raw = _raw_transform(device, host, shape, name, layout, out_layout)
  assert truth.same_bits(raw.reshape(want.shape), want)
  if shape == (1, 64, 257):
    raw = one_block(lambda: _raw_transform(device, host, shape, name, layout,
                                           out_layout))
    assert truth.same_bits(raw.reshape(want.shape), want)


def test_single_images_and_defaults(device):
  """(h, w, 3) and (3, h, w) without the count axis; rgb_to_ycbcr and
  ycbcr_to_rgb are color_transform with the JFIF constants."""
  from utils import color
  host = truth.wild_stack(1, 9, 12)
  x = helpers.to_dev(host[0], device)
  ycc = color.rgb_to_ycbcr(x)
  assert tuple(ycc.shape) == (9, 12, 3)
  assert truth.same_bits(ycc.cpu().numpy(), truth.rgb_to_ycbcr(host)[0])
  planar = color.rgb_to_ycbcr(x, 0.5, out_layout='chw')
  assert tuple(planar.shape) == (3, 9, 12)
  assert truth.same_bits(
      planar.cpu().numpy(),
      truth.rgb_to_ycbcr(host, 0.5, out_layout=truth.CHW)[0])
  back = color.ycbcr_to_rgb(planar, 0.5, clamp=(0., 1.), layout='chw',
                            out_layout='hwc')
  want = truth.ycbcr_to_rgb(planar.cpu().numpy()[None], 0.5, clamp=(0., 1.),
                            layout=truth.CHW, out_layout=truth.HWC)[0]
  assert truth.same_bits(back.cpu().numpy(), want)


@pytest.mark.parametrize('shape', PLANES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('fv', truth.FACTORS)
@pytest.mark.parametrize('fh', truth.FACTORS)
def test_plane_downsample(device, one_block, fh, fv, shape):
  from utils import color
  host = truth.plane_stack(*shape)
  want = truth.downsample(host, fv, fh)
  x = helpers.to_dev(host, device)
  got = color.subsample_plane(x, (fv, fh))
  assert tuple(got.shape) == want.shape
  assert truth.same_bits(got.cpu().numpy(), want)
  assert torch.equal(got, color.subsample_plane(x, (fv, fh)))
  capped = one_block(lambda: color.subsample_plane(x, (fv, fh)))
  assert torch.equal(got, capped)
  # one plane without the count axis
  assert torch.equal(color.subsample_plane(x[0], (fv, fh)), got[0])


@pytest.mark.parametrize('shape', OUT_SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('mode', ['replicate', 'triangle'])
@pytest.mark.parametrize('fv', truth.FACTORS)
@pytest.mark.parametrize('fh', truth.FACTORS)
def test_plane_upsample(device, one_block, fh, fv, mode, shape):
  from utils import color
  h, w = shape
  host = truth.plane_stack(2, -(-h // fv), -(-w // fh), seed=1)
  code = truth.TRIANGLE if mode == 'triangle' else truth.REPLICATE
  want = truth.upsample(host, fv, fh, shape, code)
  x = helpers.to_dev(host, device)
  got = color.upsample_plane(x, (fv, fh), shape, mode)
  assert tuple(got.shape) == (2, h, w)
  assert truth.same_bits(got.cpu().numpy(), want)
  assert torch.equal(got, color.upsample_plane(x, (fv, fh), shape, mode))
  capped = one_block(lambda: color.upsample_plane(x, (fv, fh), shape, mode))
  assert torch.equal(got, capped)
  assert torch.equal(color.upsample_plane(x[1], (fv, fh), shape, mode), got[1])
  if fv == fh == 1:
    assert torch.equal(got, x)


def test_round_trip_of_8bit_colours(device):
  from utils import color
  host = truth.colours_8bit(4096)
  x = helpers.to_dev(host, device)
  ycc = color.rgb_to_ycbcr(x)
  back = color.ycbcr_to_rgb(ycc)
  assert truth.same_bits(ycc.cpu().numpy(), truth.rgb_to_ycbcr(host))
  want = truth.ycbcr_to_rgb(truth.rgb_to_ycbcr(host))
  assert truth.same_bits(back.cpu().numpy(), want)
  assert np.array_equal(np.rint(back.cpu().numpy()), host)
  # grey: chroma is the offset exactly
  g = np.arange(256, dtype=np.float32)
  grey = helpers.to_dev(np.stack([g, g, g], axis=-1).reshape(1, 16, 16, 3),
                        device)
  ycc = color.rgb_to_ycbcr(grey).cpu().numpy()
  assert np.array_equal(ycc[..., 0].reshape(-1), g)
  assert (ycc[..., 1:] == np.float32(128.)).all()


def test_split_and_merge_planes(device):
  """split_planes and merge_planes are the transform and the resamplers put
  together; a ragged 33 x 47 image at 4:2:0 and at (4, 1)."""
  from utils import color
  host = truth.colour_image(33, 47)
  x = helpers.to_dev(host, device)
  for fv, fh in ((2, 2), (4, 1), (1, 1)):
    planes = color.split_planes(x, (fv, fh))
    ycc = truth.rgb_to_ycbcr(host[None], out_layout=truth.CHW)[0]
    small = truth.downsample(ycc[1:], fv, fh)
    assert truth.same_bits(planes[0].cpu().numpy(), ycc[0])
    assert truth.same_bits(planes[1].cpu().numpy(), small[0])
    assert truth.same_bits(planes[2].cpu().numpy(), small[1])
    for mode, code in (('triangle', truth.TRIANGLE),
                       ('replicate', truth.REPLICATE)):
      merged = color.merge_planes(planes, (33, 47), (fv, fh), upsampling=mode,
                                  clamp=(0., 255.))
      full = np.concatenate(
          [ycc[:1], truth.upsample(small, fv, fh, (33, 47), code)])
      want = truth.ycbcr_to_rgb(full[None], clamp=(0., 255.),
                                layout=truth.CHW, out_layout=truth.HWC)[0]
      assert tuple(merged.shape) == (33, 47, 3)
      assert truth.same_bits(merged.cpu().numpy(), want)
