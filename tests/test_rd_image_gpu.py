"""utils.jpeg.rate_distortion_image: a whole image through an orthonormal
dictionary, the JPEG streams and back, with bits per pixel, pSNR and SSIM
measured on the reassembled image (the reference's fullimg_reshape_params).

A 40 x 56 seeded image in [0, 255], 8 x 8 patches, the 64 x 64 DCT basis built
here from its formula, the Annex K.1 bin widths in zig-zag order.  The rate
must be rate_distortion_point's on the same patches, the two distortions
compute_pSNR's and compute_ssim's on images assembled here, and the SSIM
within 1e-9 (the bound of tests/test_ssim_gpu.py, whose +-2 R condition is
asserted) of tests/ssim_oracle.py on the images read back.
"""
import numpy as np
import pytest
import torch

import helpers
import ssim_oracle

pytestmark = pytest.mark.gpu

H, W, P = 40, 56, 8
BOUND = 1e-9


def dct_basis():
  """(64, 64) float32: row 8u + v is the 8 x 8 DCT-II basis image (u, v)
  flattened row-major, c(u) c(v) cos((2i + 1) u pi / 16) cos((2j + 1) v pi /
  16), c(0) = sqrt(1/8), c(k > 0) = sqrt(2/8).  Orthonormal."""
  k = np.arange(P)
  one_d = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / (2 * P))
  one_d *= np.where(k == 0, np.sqrt(1. / P), np.sqrt(2. / P))[:, None]
  basis = np.einsum('ui,vj->uvij', one_d, one_d).reshape(P * P, P * P)
  assert np.abs(basis @ basis.T - np.eye(P * P)).max() < 1e-12
  return basis.astype(np.float32)


def seeded_image(h=H, w=W):
  rs = np.random.RandomState(4056)
  yy, xx = np.mgrid[0:h, 0:w]
  smooth = (np.sin(yy / 5.) + np.cos(xx / 7.) + np.sin((yy + xx) / 11.)) / 3.
  image = 127.5 + 100. * smooth + 8. * rs.randn(h, w)
  return np.clip(image, 0., 255.).astype(np.float32)


@pytest.fixture(scope='module')
def setting(device):
  from utils import jpeg, matrix_zigzag
  return {'image': helpers.to_dev(seeded_image(), device),
          'dictionary': helpers.to_dev(dct_basis(), device),
          'widths': jpeg.get_jpeg_quant_hifi_binwidths(),
          'order': matrix_zigzag.scan_order(P, P)}


def _rd(setting, multiplier, image=None, **kwargs):
  from utils import jpeg
  return jpeg.rate_distortion_image(
      setting['image'] if image is None else image, setting['dictionary'],
      (P, P), setting['widths'], multiplier, order=setting['order'], **kwargs)


def _patches(image):
  from utils import image_processing
  return image_processing.patches_from_single_image(image[:, :, None], (P, P),
                                                    flatten_patches=True)


@pytest.mark.parametrize('multiplier', [1.0, 4.0])
def test_rate_is_that_of_rate_distortion_point(setting, multiplier):
  from utils import jpeg
  patches, _ = _patches(setting['image'])
  assert tuple(patches.shape) == (35, 64)
  bpp, _, tables = jpeg.rate_distortion_point(
      patches, setting['dictionary'], setting['widths'], multiplier,
      order=setting['order'])
  trained = _rd(setting, multiplier)
  assert sorted(trained) == ['SSIM', 'bits_per_pixel', 'pSNR', 'tables']
  assert trained['tables'] == tables
  assert trained['bits_per_pixel'] == bpp
  given = _rd(setting, multiplier, tables=tables)
  assert given['tables'] is tables and given['bits_per_pixel'] == bpp
  assert given['pSNR'] == trained['pSNR'] and given['SSIM'] == trained['SSIM']


@pytest.mark.parametrize('mean', [None, 128.0])
def test_distortions_are_those_of_the_assembled_images(setting, device, mean):
  from analysis_transforms.fully_connected import invertible_linear
  from utils import image_processing, jpeg, plotting
  multiplier = 2.0
  means = None if mean is None else np.full(P * P, mean, dtype=np.float32)
  result = _rd(setting, multiplier, component_means=means)
  # by hand: the same calls, the images assembled here
  patches, positions = _patches(setting['image'])
  coded = patches
  if means is not None:
    coded = patches - helpers.to_dev(means, device)
  widths = setting['widths'] * multiplier
  levels = jpeg.quantize(
      invertible_linear.run(coded, setting['dictionary']), widths,
      setting['order'])
  back = invertible_linear.apply_filter(
      jpeg.dequantize(levels, widths, setting['order']),
      setting['dictionary'])
  if means is not None:
    back = back + helpers.to_dev(means, device)
  original = image_processing.assemble_image_from_patches(
      patches, (P, P), positions)[:, :, 0]
  rebuilt = image_processing.assemble_image_from_patches(
      back, (P, P), positions)[:, :, 0]
  assert torch.equal(original, setting['image'])
  assert result['pSNR'] == plotting.compute_pSNR(original, rebuilt)
  assert result['SSIM'] == plotting.compute_ssim(original, rebuilt)
  bits = jpeg.stream_bits(levels, *result['tables'])
  assert result['bits_per_pixel'] == int(bits.sum()) / float(H * W)
  # truth: float64 on the images read back
  x, y = original.cpu().numpy(), rebuilt.cpu().numpy()
  r = ssim_oracle.derived_range(x)
  assert max(np.abs(x).max(), np.abs(y).max()) <= 2 * r
  want, _ = ssim_oracle.ssim(x, y)
  print('rd_image mean %s: bpp %.4f pSNR %.3f SSIM %.12f (off by %.2e)'
        % (mean, result['bits_per_pixel'], result['pSNR'], result['SSIM'],
           abs(result['SSIM'] - want)))
  assert abs(result['SSIM'] - want) <= BOUND
  assert 0.5 < result['SSIM'] < 1.0 and 20 < result['pSNR'] < 80


def test_fine_quantisation_is_nearly_lossless(setting):
  coarse, fine = _rd(setting, 8.0), _rd(setting, 0.01)
  assert fine['SSIM'] > 0.999
  assert fine['SSIM'] > coarse['SSIM'] and fine['pSNR'] > coarse['pSNR']
  assert fine['bits_per_pixel'] > coarse['bits_per_pixel']


def test_only_the_covered_part_is_measured(setting, device):
  """43 x 59: three rows and three columns beyond the last whole patch, filled
  with values that would move every figure."""
  larger = torch.full((43, 59), 1000., dtype=torch.float32, device=device)
  larger[:H, :W] = setting['image']
  want = _rd(setting, 2.0)
  got = _rd(setting, 2.0, image=larger)
  for key in ('bits_per_pixel', 'pSNR', 'SSIM', 'tables'):
    assert got[key] == want[key], key


def test_zero_means_change_nothing(setting, device):
  want = _rd(setting, 2.0)
  for zeros in (np.zeros(P * P, dtype=np.float32),
                torch.zeros(P * P, device=device)):
    got = _rd(setting, 2.0, component_means=zeros)
    for key in ('bits_per_pixel', 'pSNR', 'SSIM', 'tables'):
      assert got[key] == want[key], key
  with pytest.raises(ValueError):
    _rd(setting, 2.0, component_means=np.zeros(63, dtype=np.float32))
