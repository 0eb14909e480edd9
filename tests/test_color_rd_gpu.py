"""utils.color.rate_distortion_image_color: a colour image split into Y, Cb and
Cr, each plane through the orthonormal 8 x 8 DCT, the JPEG streams and back,
merged and measured on the image.

Two seeded smooth-plus-noise images in [0, 255] (tests/color_data.py): 33 x 47,
of which 4:2:0 with 8 x 8 patches covers 32 x 32 (two MCUs each way, chroma
planes 16 x 16), and 48 x 64 (chroma planes 24 x 32, large enough for the 11
tap SSIM window of rate_distortion_image).  Annex K.1 and K.2 bin widths in
zig-zag order, a level shift of 128.  Every figure is compared with the same
steps taken one at a time through the public functions: equal integers, equal
floats, equal bit patterns.
"""
import numpy as np
import pytest
import torch

import color_data as truth
import helpers

pytestmark = pytest.mark.gpu

P = 8
SHIFT = 128.0
KEYS = ['SSIM_Y', 'bits', 'bits_per_pixel', 'pSNR', 'pSNR_Y', 'reconstruction',
        'tables']


@pytest.fixture(scope='module')
def setting(device):
  from utils import jpeg
  return {'small': helpers.to_dev(truth.colour_image(33, 47), device),
          'large': helpers.to_dev(truth.colour_image(48, 64, seed=4864),
                                  device),
          'dictionary': helpers.to_dev(truth.dct_basis(P), device),
          'luma': jpeg.get_jpeg_quant_hifi_binwidths(),
          'chroma': jpeg.get_jpeg_quant_chroma_binwidths(),
          'order': truth.scan_order(P)}


def _rd(setting, image, multiplier=1.0, **kwargs):
  from utils import color
  kwargs.setdefault('level_shift', SHIFT)
  return color.rate_distortion_image_color(
      setting[image], setting['dictionary'], (P, P), setting['luma'],
      setting['chroma'], multiplier, order=setting['order'], **kwargs)


@pytest.fixture(scope='module')
def point420(setting):
  return _rd(setting, 'small')


def _by_hand(setting, image, H, W, subsampling, multiplier, tables=None,
             upsampling='triangle', clamp=None):
  """The steps of the R-D point one at a time through the public functions.
  Returns (planes, levels, counts, tables, bits, decoded planes)."""
  from analysis_transforms.fully_connected import invertible_linear
  from utils import color, image_processing, jpeg
  device = setting[image].device
  planes = color.split_planes(setting[image][:H, :W].contiguous(), subsampling)
  shift = torch.full((P * P,), SHIFT, dtype=torch.float32, device=device)
  levels, positions, counts = [], [], []
  for plane, widths in zip(planes, (setting['luma'], setting['chroma'],
                                    setting['chroma'])):
    patches, where = image_processing.patches_from_single_image(
        plane[:, :, None], (P, P), flatten_patches=True)
    codes = invertible_linear.run(patches - shift, setting['dictionary'])
    levels.append(jpeg.quantize(codes, widths * multiplier, setting['order']))
    positions.append(where)
    counts.append(jpeg.symbol_counts(levels[-1]))
  if tables is None:
    tables = (jpeg.tables_from_counts(*counts[0]),
              jpeg.tables_from_counts(counts[1][0] + counts[2][0],
                                      counts[1][1] + counts[2][1]))
  bits, decoded = [], []
  for lv, where, widths, pair in zip(
      levels, positions,
      (setting['luma'], setting['chroma'], setting['chroma']),
      (tables[0], tables[1], tables[1])):
    packed, offsets = jpeg.pack_streams(lv, pair[0], pair[1])
    bits.append(int(offsets[-1]))
    back = jpeg.decode_patches(packed, offsets, setting['dictionary'], widths,
                               multiplier, pair, setting['order'])
    decoded.append(image_processing.assemble_image_from_patches(
        back + shift, (P, P), where)[:, :, 0])
  return planes, levels, counts, tables, bits, decoded


def test_420_rates_and_tables(setting, point420):
  from utils import jpeg
  assert sorted(point420) == KEYS
  assert all(type(b) is int for b in point420['bits'])
  planes, levels, counts, tables, bits, _ = _by_hand(
      setting, 'small', 32, 32, (2, 2), 1.0)
  assert [tuple(p.shape) for p in planes] == [(32, 32), (16, 16), (16, 16)]
  # luma: the grey R-D point of the cropped Y plane, with its own tables
  grey = jpeg.rate_distortion_image(
      planes[0], setting['dictionary'], (P, P), setting['luma'], 1.0,
      order=setting['order'],
      component_means=np.full(P * P, SHIFT, dtype=np.float32))
  assert point420['tables'][0] == grey['tables']
  assert point420['bits'][0] == grey['bits_per_pixel'] * 32 * 32
  # chroma: one pair trained on the sum of both planes' counts
  assert point420['tables'][1] == jpeg.tables_from_counts(
      counts[1][0] + counts[2][0], counts[1][1] + counts[2][1])
  assert point420['tables'] == tables
  assert list(point420['bits']) == bits
  for i in (1, 2):
    assert point420['bits'][i] == int(jpeg.stream_bits(
        levels[i], *tables[1]).sum())
  assert point420['bits_per_pixel'] == sum(bits) / float(32 * 32)
  assert 0.1 < point420['bits_per_pixel'] < 12.0


def test_chroma_rates_are_those_of_the_grey_route(setting):
  """48 x 64: the 24 x 32 chroma planes are large enough for
  rate_distortion_image, which is given the shared chroma tables."""
  from utils import color, jpeg
  point = _rd(setting, 'large')
  planes = color.split_planes(setting['large'], (2, 2))
  assert [tuple(p.shape) for p in planes] == [(48, 64), (24, 32), (24, 32)]
  means = np.full(P * P, SHIFT, dtype=np.float32)
  for i, widths, pair in ((0, setting['luma'], point['tables'][0]),
                          (1, setting['chroma'], point['tables'][1]),
                          (2, setting['chroma'], point['tables'][1])):
    grey = jpeg.rate_distortion_image(
        planes[i], setting['dictionary'], (P, P), widths, 1.0, tables=pair,
        order=setting['order'], component_means=means)
    assert point['bits'][i] / float(planes[i].numel()) == (
        grey['bits_per_pixel']), i
  assert point['bits_per_pixel'] == sum(point['bits']) / float(48 * 64)


@pytest.mark.parametrize('upsampling,clamp', [('triangle', None),
                                              ('replicate', (0., 255.))])
def test_420_reconstruction_and_distortions(setting, upsampling, clamp):
  from utils import color, plotting
  point = _rd(setting, 'small', 2.0, upsampling=upsampling, clamp=clamp)
  planes, _, _, tables, bits, decoded = _by_hand(
      setting, 'small', 32, 32, (2, 2), 2.0)
  assert point['tables'] == tables and list(point['bits']) == bits
  rebuilt = color.merge_planes(decoded, (32, 32), (2, 2), 128.0, upsampling,
                               clamp)
  got = point['reconstruction']
  assert tuple(got.shape) == (32, 32, 3) and got.dtype == torch.float32
  assert torch.equal(got.view(torch.int32), rebuilt.view(torch.int32))
  original = setting['small'][:32, :32].contiguous()
  assert point['pSNR'] == plotting.compute_pSNR(original, rebuilt,
                                                manual_sig_mag=255.0)
  assert point['pSNR_Y'] == plotting.compute_pSNR(planes[0], decoded[0],
                                                  manual_sig_mag=255.0)
  assert point['SSIM_Y'] == plotting.compute_ssim(planes[0], decoded[0],
                                                  manual_sig_mag=255.0)
  assert 20 < point['pSNR'] < 60 and 0.5 < point['SSIM_Y'] < 1.0
  if clamp is not None:
    assert float(got.min()) >= 0. and float(got.max()) <= 255.
  # and the restatement agrees on the merge of the decoded planes
  host = [p.cpu().numpy() for p in decoded]
  code = truth.TRIANGLE if upsampling == 'triangle' else truth.REPLICATE
  full = np.concatenate([host[0][None], truth.upsample(
      np.stack(host[1:]), 2, 2, (32, 32), code)])
  want = truth.ycbcr_to_rgb(full[None], clamp=clamp, layout=truth.CHW,
                            out_layout=truth.HWC)[0]
  assert truth.same_bits(got.cpu().numpy(), want)


def test_only_whole_mcus_are_measured(setting, device, point420):
  """33 x 47 against its 32 x 32 crop, and against the crop surrounded by
  values that would move every figure."""
  from utils import color
  cropped = setting['small'][:32, :32].contiguous()
  larger = torch.full((47, 47, 3), 1000., dtype=torch.float32, device=device)
  larger[:32, :32] = cropped
  for image in (cropped, larger):
    got = color.rate_distortion_image_color(
        image, setting['dictionary'], (P, P), setting['luma'],
        setting['chroma'], 1.0, order=setting['order'], level_shift=SHIFT)
    for key in ('bits', 'bits_per_pixel', 'pSNR', 'pSNR_Y', 'SSIM_Y',
                'tables'):
      assert got[key] == point420[key], key
    assert torch.equal(got['reconstruction'], point420['reconstruction'])


def test_444(setting):
  """subsampling (1, 1): the chroma planes are coded at full size (32 x 40 of
  the 33 x 47 image is covered) and merge_planes is the plain inverse
  transform of the decoded planes."""
  from utils import color
  point = _rd(setting, 'small', subsampling=(1, 1))
  planes, _, _, tables, bits, decoded = _by_hand(
      setting, 'small', 32, 40, (1, 1), 1.0)
  assert [tuple(p.shape) for p in planes] == [(32, 40)] * 3
  assert point['tables'] == tables and list(point['bits']) == bits
  assert point['bits_per_pixel'] == sum(bits) / float(32 * 40)
  plain = color.ycbcr_to_rgb(torch.stack(decoded), layout='chw',
                             out_layout='hwc')
  for upsampling in ('triangle', 'replicate'):
    got = _rd(setting, 'small', subsampling=(1, 1), upsampling=upsampling)
    assert torch.equal(got['reconstruction'].view(torch.int32),
                       plain.view(torch.int32))


def test_grey_image_has_dc_only_chroma(setting, device):
  from utils import color, jpeg
  grey = setting['small'][:, :, :1].expand(33, 47, 3).contiguous()
  planes, levels, _, _, _, _ = _by_hand(
      dict(setting, grey=grey), 'grey', 32, 32, (2, 2), 1.0)
  assert torch.equal(planes[0], grey[:32, :32, 0])
  for plane, lv in zip(planes[1:], levels[1:]):
    assert bool((plane == 128.).all())
    assert bool((lv[:, 1:] == 0).all())
    assert bool((lv[:, 0] == 0).all())   # 128 less the level shift
  # without the level shift the DC level carries the offset, and only it
  shift0 = color.rate_distortion_image_color(
      grey, setting['dictionary'], (P, P), setting['luma'], setting['chroma'],
      1.0, order=setting['order'])
  widths = setting['chroma']
  from analysis_transforms.fully_connected import invertible_linear
  from utils import image_processing
  patches, _ = image_processing.patches_from_single_image(
      planes[1][:, :, None], (P, P), flatten_patches=True)
  raw = jpeg.quantize(invertible_linear.run(patches, setting['dictionary']),
                      widths, setting['order'])
  assert bool((raw[:, 0] == round(128. * 8 / widths[0])).all())
  assert bool((raw[:, 1:] == 0).all())
  # Cb and Cr are one plane twice: the same streams
  assert shift0['bits'][1] == shift0['bits'][2] > 0


def test_coarser_quantisation_costs_less_and_shows(setting, point420):
  coarse = _rd(setting, 'small', 8.0)
  for fine_bits, coarse_bits in zip(point420['bits'], coarse['bits']):
    assert coarse_bits <= fine_bits
  assert coarse['bits_per_pixel'] <= point420['bits_per_pixel']
  assert coarse['pSNR'] <= point420['pSNR']


def test_given_tables_reproduce_the_bits(setting, point420):
  again = _rd(setting, 'small', tables=point420['tables'])
  assert again['tables'] is point420['tables']
  for key in ('bits', 'bits_per_pixel', 'pSNR', 'pSNR_Y', 'SSIM_Y'):
    assert again[key] == point420[key], key
  assert torch.equal(again['reconstruction'], point420['reconstruction'])
  # another multiplier under the same tables: other bits, same tables
  other = _rd(setting, 'small', 4.0, tables=point420['tables'])
  assert other['tables'] is point420['tables']
  assert other['bits'] != point420['bits']
