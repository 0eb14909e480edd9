"""The image-level half of utils.image_processing on the MI355X
(csrc/image_tools.hip, include/vtc_image.h) against the reference's outputs in
tests/golden/image_tools.npz (tools/make_golden_image_tools.py).

Bounds.  Moves (downsample, tiling, assembling) are torch.equal to the
reference's arrays.  The float64-then-cast routes (filter_fd, filter_sd,
unwhiten_center_surround) are held to helpers.rel_err < 1e-6, the bound
tests/test_patches_gpu.py uses for the same construction; the recorder checked
that an independent float64 numpy statement of every case stays inside it
against the reference (the 1 / F cases come closest, 7.5e-7: this numpy runs
the reference's forward transform of a float32 image in single precision, and
the inverse gain of up to 1e3 multiplies that).  Every route run twice is
bit-equal.
"""
import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

BOUND = 1e-6


@pytest.fixture(scope='module')
def g():
  return helpers.load('image_tools')


def _ip():
  from utils import image_processing as ip
  return ip


def _dev(a, device):
  return helpers.to_dev(a, device)


def _close(got, want, what):
  assert got.is_cuda and got.dtype == torch.float32, what
  got = got.cpu().numpy()
  assert got.shape == want.shape, what
  err = helpers.rel_err(got, want)
  print('image_tools %-36s rel err %.3e' % (what, err))
  assert err < BOUND, '%s: rel err %.3e' % (what, err)


def _twice(fn):
  a, b = fn(), fn()
  torch.cuda.synchronize()
  if isinstance(a, tuple):
    a, b = a[0], b[0]
  assert torch.equal(a, b)
  return a


# ---- filter_fd ---------------------------------------------------------------
@pytest.mark.parametrize('kind', ['lp', 'cx'])
@pytest.mark.parametrize('shape', ['37x53', '40x64', '41x55'])
def test_filter_fd(device, g, kind, shape):
  ip = _ip()
  filt = g['fd_%s_filter_%s' % (kind, shape)]
  img = _dev(g['img'][0], device)
  out = _twice(lambda: ip.filter_fd(img, filt))
  _close(out, g['fd_%s_%s_img0' % (kind, shape)], 'filter_fd ' + kind + shape)
  # a device filter is the same call
  assert torch.equal(ip.filter_fd(img, _dev(filt, device)), out)


def test_filter_fd_low_pass_builder_matches_the_reference(g):
  ip = _ip()
  for shape in ((37, 53), (40, 64), (41, 55)):
    ours = ip.get_low_pass_filter(
        shape, {'shape': 'exponential', 'cutoff': 0.3, 'order': 4.0})
    ref = g['fd_lp_filter_%dx%d' % shape]
    assert ours.dtype == np.complex128 and ours.shape == shape
    assert np.abs(ours - ref).max() <= 1e-15


def test_filter_fd_non_hermitian_filter_is_not_symmetric(g):
  """The complex case of the fixture really is one a D2Z / Z2D pair that
  ignored F[-k] would get wrong."""
  f = g['fd_cx_filter_40x64']
  mirrored = np.roll(f[::-1, ::-1], (1, 1), axis=(0, 1))
  assert np.abs(f - np.conj(mirrored)).max() > 1.0


def test_filter_fd_stack_equals_per_image_calls(device, g):
  ip = _ip()
  filt = g['fd_lp_filter_37x53']
  stack = _dev(g['img'], device)
  out = _twice(lambda: ip.filter_fd(stack, filt))
  assert out.shape == stack.shape
  for i in range(2):
    assert torch.equal(out[i], ip.filter_fd(stack[i], filt))
    _close(out[i], g['fd_lp_37x53_img%d' % i], 'filter_fd stack %d' % i)
  cx = g['fd_cx_filter_40x64']
  both = ip.filter_fd(stack, cx)
  for i in range(2):
    assert torch.equal(both[i], ip.filter_fd(stack[i], cx))


def test_filter_fd_uint8(device, g):
  ip = _ip()
  img = _dev(g['img_u8'][0], device)
  out = _twice(lambda: ip.filter_fd(img, g['fd_cx_filter_40x64']))
  _close(out, g['fd_cx_40x64_u8'], 'filter_fd uint8')


def test_filter_fd_refuses_an_undersampled_filter(device, g):
  ip = _ip()
  img = _dev(g['img'][0], device)
  with pytest.raises(AssertionError):
    ip.filter_fd(img, np.ones((36, 53), dtype=np.complex128))


# ---- filter_sd ---------------------------------------------------------------
@pytest.mark.parametrize('tag', ['5x7', '4x6', '1x1', '37x3'])
def test_filter_sd_general(device, g, tag):
  ip = _ip()
  img = _dev(g['img'][0], device)
  filt = g['sd_filter_' + tag]
  out = _twice(lambda: ip.filter_sd(img, filt))
  _close(out, g['sd_%s_img0' % tag], 'filter_sd ' + tag)
  assert torch.equal(ip.filter_sd(img, _dev(filt, device)), out)


def test_filter_sd_general_is_a_convolution_of_this_filter(g):
  """The 5 x 7 taps are all distinct and the filter is neither symmetric nor
  square: a correlation or a transposed filter cannot reproduce the fixture."""
  f = g['sd_filter_5x7']
  assert len(np.unique(f)) == f.size
  assert np.abs(f - f[::-1, ::-1]).max() > 0.1


def test_filter_sd_stack_and_uint8(device, g):
  ip = _ip()
  filt = g['sd_filter_5x7']
  stack = _dev(g['img'], device)
  out = _twice(lambda: ip.filter_sd(stack, filt))
  for i in range(2):
    assert torch.equal(out[i], ip.filter_sd(stack[i], filt))
  _close(out[0], g['sd_5x7_img0'], 'filter_sd stack 0')
  u8 = _dev(g['img_u8'][0], device)
  _close(_twice(lambda: ip.filter_sd(u8, filt)), g['sd_5x7_u8'],
         'filter_sd uint8')


@pytest.mark.parametrize('tag', ['img0', 'u8'])
def test_filter_sd_separable(device, g, tag):
  ip = _ip()
  img = _dev(g['img'][0] if tag == 'img0' else g['img_u8'][0], device)
  out = _twice(lambda: ip.filter_sd(img, None, separable_vert=g['sd_vert'],
                                    separable_horz=g['sd_horz']))
  _close(out, g['sd_separable_' + tag], 'filter_sd separable ' + tag)


def test_filter_sd_separable_keeps_the_intermediate_rounding(device, g):
  """The outer product of the two factors through the general route differs
  from the separable route: the horizontal pass was stored as float32."""
  ip = _ip()
  img = _dev(g['img'][0], device)
  outer = g['sd_vert'][:, None] * g['sd_horz'][None, :]
  general = ip.filter_sd(img, outer).cpu().numpy()
  want = g['sd_separable_img0']
  assert helpers.rel_err(general, want) < 1e-6
  assert not np.array_equal(general, want)


def test_filter_sd_multi_tile_image(device):
  """More than one tile in both axes with a ragged edge, a 63-tap filter
  (the largest LDS tile) against the float64 statement."""
  ip = _ip()
  rs = np.random.RandomState(5)
  img = rs.rand(70, 150, 1).astype(np.float32)
  filt = rs.randn(63, 9) / 63
  out = _twice(lambda: ip.filter_sd(_dev(img, device), filt)).cpu().numpy()
  padded = np.pad(img[:, :, 0].astype(np.float64), ((31, 31), (4, 4)),
                  mode='symmetric')
  want = np.zeros((70, 150))
  for j in range(63):
    for i in range(9):
      want += filt[j, i] * padded[62 - j:62 - j + 70, 8 - i:8 - i + 150]
  assert helpers.rel_err(out[:, :, 0], want.astype(np.float32)) < BOUND


@pytest.mark.parametrize('shape', [(64, 3), (3, 64), (38, 3), (3, 54)])
def test_filter_sd_unsupported_sizes(device, g, shape):
  ip = _ip()
  big = np.zeros((80, 80, 1), dtype=np.float32)
  img = _dev(big if max(shape) == 64 else g['img'][0], device)
  with pytest.raises(NotImplementedError):
    ip.filter_sd(img, np.ones(shape))
  with pytest.raises(NotImplementedError):
    ip.filter_sd(img, None, separable_vert=np.ones(shape[0]),
                 separable_horz=np.ones(shape[1]))


# ---- downsample ---------------------------------------------------------------
@pytest.mark.parametrize('factor', [1, 2, 3, 5])
def test_downsample(device, g, factor):
  ip = _ip()
  for key, suffix in (('img', ''), ('img_u8', '_u8')):
    want = torch.from_numpy(g['down_%d%s' % (factor, suffix)])
    img = _dev(g[key][0], device)
    out = _twice(lambda: ip.downsample(img, factor))
    assert out.dtype == want.dtype and torch.equal(out.cpu(), want)
    stack = ip.downsample(_dev(g[key], device), factor)
    assert torch.equal(stack[0], out)
    assert torch.equal(stack[1].cpu(),
                       torch.from_numpy(g[key][1][::factor, ::factor].copy()))


# ---- tiling -------------------------------------------------------------------
def test_tile_with_overflow(device, g, capsys):
  ip = _ip()
  img = _dev(g['img'][0], device)
  patches, positions = _twice_pair(lambda: ip.patches_from_single_image(
      img, (8, 8), False))
  assert 'Warning: image cannot be completely patched' in capsys.readouterr().out
  assert torch.equal(patches.cpu(), torch.from_numpy(g['tile_8x8']))
  assert positions == [tuple(int(v) for v in p)
                       for p in g['tile_8x8_positions']]
  flat, _ = ip.patches_from_single_image(img, (8, 8), True)
  assert torch.equal(flat, patches.reshape(patches.shape[0], -1))
  u8, _ = ip.patches_from_single_image(_dev(g['img_u8'][0], device), (8, 8),
                                       True)
  assert u8.dtype == torch.uint8
  assert torch.equal(u8.cpu(), torch.from_numpy(g['tile_8x8_u8']))
  stack, _ = ip.patches_from_single_image(_dev(g['img'], device), (8, 8),
                                          False)
  assert torch.equal(stack[0], patches)
  assert torch.equal(stack[1], ip.patches_from_single_image(
      _dev(g['img'][1], device), (8, 8), False)[0])


def _twice_pair(fn):
  (a, pa), (b, pb) = fn(), fn()
  torch.cuda.synchronize()
  assert torch.equal(a, b) and pa == pb
  return a, pa


def test_tile_exact_and_back(device, g, capsys):
  ip = _ip()
  img = _dev(g['exact_img'], device)
  patches, positions = _twice_pair(lambda: ip.patches_from_single_image(
      img, (16, 16), True))
  assert 'Warning' not in capsys.readouterr().out
  assert torch.equal(patches.cpu(), torch.from_numpy(g['tile_16x16']))
  back = _twice(lambda: ip.assemble_image_from_patches(patches, (16, 16),
                                                       positions))
  assert torch.equal(back, img)


def test_assemble_permuted_positions(device, g):
  ip = _ip()
  tiles = _dev(g['tile_8x8'], device)
  pos = [tuple(int(v) for v in p) for p in g['tile_8x8_positions']]
  perm = g['assemble_perm']
  out = _twice(lambda: ip.assemble_image_from_patches(
      tiles[torch.from_numpy(perm).long().to(device)], (8, 8),
      [pos[i] for i in perm]))
  assert torch.equal(out.cpu(), torch.from_numpy(g['assemble_perm_image']))


def test_assemble_subset_leaves_holes_zero(device, g):
  ip = _ip()
  tiles = _dev(g['tile_8x8'], device)
  pos = [tuple(int(v) for v in p) for p in g['tile_8x8_positions']]
  subset = g['assemble_subset']
  chosen = tiles[torch.from_numpy(subset).long().to(device)]
  out = _twice(lambda: ip.assemble_image_from_patches(
      chosen.reshape(len(subset), -1), (8, 8), [pos[i] for i in subset]))
  want = g['assemble_subset_image']
  assert (want == 0).any()
  assert torch.equal(out.cpu(), torch.from_numpy(want))


def test_assemble_overlapping_positions_keep_the_later_patch(device, g):
  ip = _ip()
  pos = [tuple(int(v) for v in p) for p in g['assemble_overlap_positions']]
  for key, suffix in (('tile_8x8', ''), ('tile_8x8_u8', '_u8')):
    tiles = _dev(g[key][:len(pos)], device)
    out = _twice(lambda: ip.assemble_image_from_patches(tiles, (8, 8), pos))
    want = torch.from_numpy(g['assemble_overlap_image' + suffix])
    assert out.dtype == want.dtype and torch.equal(out.cpu(), want)


def test_disjoint_check_of_the_position_table():
  ip = _ip()
  grid = np.array([(i * 8, j * 8) for i in range(4) for j in range(6)])
  assert ip._positions_disjoint(grid, 8, 8, 32, 48)
  assert ip._positions_disjoint(grid[::-1], 8, 8, 32, 48)
  touching = np.array([(0, 0), (7, 8), (8, 0)])
  assert ip._positions_disjoint(touching, 8, 8, 16, 16)
  assert not ip._positions_disjoint(np.array([(0, 0), (7, 7)]), 8, 8, 15, 15)
  assert not ip._positions_disjoint(np.array([(3, 3), (3, 3)]), 8, 8, 11, 11)


# ---- unwhiten_center_surround, compute_pSNR ------------------------------------
@pytest.mark.parametrize('tag,low', [('low0', 0.0), ('low1e-3', 1e-3)])
def test_unwhiten_center_surround_exact(device, g, tag, low):
  ip = _ip()
  cutoffs = {'low': low, 'high': 0.8}
  filt = ip.center_surround_filter((64, 48, 1), cutoffs)
  assert filt.dtype == np.complex128 and filt.shape == (64, 48)
  assert np.abs(1. / filt).max() <= 1e3 * (1 + 1e-12)
  natural = _dev(g['natural'], device)
  # the device whitening and the host filter describe the same transform
  white = ip.whiten_center_surround(natural, cutoffs)
  _close(white, g['white_' + tag], 'whiten ' + tag)
  _close(ip.filter_fd(natural, filt), g['white_' + tag], 'filter_fd F ' + tag)
  ref_white = _dev(g['white_' + tag], device)
  out = _twice(lambda: ip.unwhiten_center_surround(ref_white,
                                                   orig_filter_DFT=filt))
  _close(out, g['unwhite_exact_' + tag], 'unwhiten exact ' + tag)
  assert torch.equal(out, ip.unwhiten_center_surround(
      ref_white, orig_filter_DFT=_dev(filt, device)))


def test_unwhiten_center_surround_ramp(device, g):
  ip = _ip()
  white = _dev(g['white_low0'], device)
  out = _twice(lambda: ip.unwhiten_center_surround(
      white, low_cutoff=float(g['low_cutoff'])))
  _close(out, g['unwhite_ramp'], 'unwhiten ramp')
  stack = ip.unwhiten_center_surround(torch.stack([white, white]),
                                      low_cutoff=float(g['low_cutoff']))
  assert torch.equal(stack[0], out) and torch.equal(stack[1], out)


def test_unwhiten_center_surround_keeps_the_reference_asserts(device, g):
  ip = _ip()
  white = _dev(g['white_low0'], device)
  with pytest.raises(AssertionError):
    ip.unwhiten_center_surround(white)
  with pytest.raises(AssertionError):
    ip.unwhiten_center_surround(white.to(torch.uint8), low_cutoff=0.05)


def test_compute_psnr(device, g):
  """Within 1e-4 dB of the reference's value.  The device sums the squared
  float32 differences over rows of 4096 elements (16 per thread, then a
  tree) and the rows in float64: at most about 30 * 2^-24 = 2e-6 relative,
  1e-5 dB; the reference's own float32 pairwise mean and float32 logarithm
  are of the same size."""
  from utils import plotting
  natural = _dev(g['natural'], device)
  for key, ref in (('unwhite_ramp', 'psnr_ramp'),
                   ('unwhite_exact_low0', 'psnr_exact_low0'),
                   ('unwhite_exact_low1e-3', 'psnr_exact_low1e-3')):
    got = plotting.compute_pSNR(natural, _dev(g[key], device))
    assert isinstance(got, float)
    print('image_tools pSNR %-24s %.6f reference %.6f' % (key, got,
                                                         float(g[ref])))
    assert abs(got - float(g[ref])) <= 1e-4
  got = plotting.compute_pSNR(natural, _dev(g['unwhite_ramp'], device),
                              manual_sig_mag=1.0)
  assert abs(got - float(g['psnr_ramp_manual'])) <= 1e-4
  assert plotting.compute_pSNR(natural, natural.clone()) == np.inf


# ---- the example's round trip -----------------------------------------------------
def test_zca_round_trip_through_tiling(device, g):
  """patches_from_single_image -> whiten_ZCA (stored parameters) -> assemble
  -> unwhiten_ZCA -> assemble, against the reference's images at the tolerance
  tests/test_zca_gpu.py holds these two transforms to (5e-6)."""
  ip = _ip()
  zca = helpers.load('zca')
  params = {'PCA_basis': zca['n64_basis'],
            'PCA_axis_variances': zca['n64_variances'],
            'subtracted_mean': zca['n64_mean']}
  natural = _dev(g['natural'], device)
  patches, positions = ip.patches_from_single_image(natural, (8, 8), True)
  white = ip.whiten_ZCA(patches, params)
  white_image = ip.assemble_image_from_patches(white, (8, 8), positions)
  recovered = ip.assemble_image_from_patches(
      ip.unwhiten_ZCA(white, params), (8, 8), positions)
  for got, key in ((white_image, 'zca_white_image'),
                   (recovered, 'zca_recovered_image')):
    err = helpers.rel_err(got.cpu().numpy(), g[key])
    print('image_tools %-36s rel err %.3e' % (key, err))
    assert err <= 5e-6
