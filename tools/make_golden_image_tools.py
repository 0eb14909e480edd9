"""
Writes tests/golden/image_tools.npz by running the REFERENCE's filter_fd,
filter_sd, downsample, patches_from_single_image, assemble_image_from_patches,
unwhiten_center_surround (utils/image_processing.py) and compute_pSNR
(utils/plotting.py) on seeded numpy.random.RandomState inputs.  The file holds
the inputs, the filters and the reference's outputs.

Before an output of a float64-then-cast route is stored, an independent
float64 numpy statement of the same case (real FFT pair with the filter's
Hermitian part; explicit symmetric padding and a tap loop) must agree with it
to helpers.rel_err < 1e-6, the bound tests/test_image_tools_gpu.py holds the
device to.  The script fails otherwise; the remedy is another filter (a higher
floor under 1 / F), never another bound.

Development-container only: it imports the reference tree (absent on the GPU
machines) with the shims of oracle/make_golden.py.  Deterministic.

  python tools/make_golden_image_tools.py
"""
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'tests'))
sys.path.insert(0, str(REPO / 'oracle'))
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

import helpers  # noqa: E402
import make_golden  # noqa: E402
import zca_data  # noqa: E402

BOUND = 1e-6
H, W, C = 37, 53, 2
FD_SHAPES = [(37, 53), (40, 64), (41, 55)]


# ---- float64 statements, independent of the reference's code path ---------
def truth_filter_fd(image, filter_dft):
  fh, fw = filter_dft.shape
  mirrored = np.roll(filter_dft[::-1, ::-1], (1, 1), axis=(0, 1))
  herm = 0.5 * (filter_dft + np.conj(mirrored))[:, :fw // 2 + 1]
  out = np.empty(image.shape, dtype=np.float64)
  for ch in range(image.shape[2]):
    spec = np.fft.rfft2(image[:, :, ch].astype(np.float64), (fh, fw))
    out[:, :, ch] = np.fft.irfft2(spec * herm, (fh, fw))[:image.shape[0],
                                                         :image.shape[1]]
  return out


def _reflect_index(i, n):
  m = np.mod(i, 2 * n)
  return np.where(m < n, m, 2 * n - 1 - m)


def truth_convolve_axis(x, taps, axis, centre):
  """sum_j taps[j] x[i + centre - j] along `axis`, symmetric reflection."""
  n = x.shape[axis]
  out = np.zeros(x.shape, dtype=np.float64)
  for j, t in enumerate(taps):
    idx = _reflect_index(np.arange(n) + centre - j, n)
    out += float(t) * np.take(x, idx, axis=axis)
  return out


def truth_filter_sd(image, filt):
  fh, fw = filt.shape
  x = image.astype(np.float64)
  out = np.zeros(x.shape, dtype=np.float64)
  for j in range(fh):
    rows = _reflect_index(np.arange(x.shape[0]) + (fh - 1) // 2 - j,
                          x.shape[0])
    out += truth_convolve_axis(x[rows], filt[j], 1, (fw - 1) // 2)
  return out


def truth_filter_sd_separable(image, vert, horz):
  mid = truth_convolve_axis(image.astype(np.float64), horz, 1, len(horz) // 2)
  mid = mid.astype(image.dtype)     # scipy stores in the input's type
  return truth_convolve_axis(mid.astype(np.float64), vert, 0, len(vert) // 2)


def checked(name, reference_output, truth):
  err = helpers.rel_err(truth.astype(np.float32), reference_output)
  print('%-28s float64 statement vs reference %.2e' % (name, err))
  assert err < BOUND, '%s: %.3e is not inside %.0e' % (name, err, BOUND)
  return reference_output


def main():
  ref = make_golden.import_reference()
  import importlib
  ip = ref.image_processing
  plotting = importlib.import_module('utils.plotting')
  rs = np.random.RandomState(20241)
  out = {}

  img = rs.rand(2, H, W, C).astype(np.float32)
  img_u8 = rs.randint(0, 256, size=(2, H, W, C)).astype(np.uint8)
  out['img'] = img
  out['img_u8'] = img_u8

  # ---- filter_fd ------------------------------------------------------------
  for fh, fw in FD_SHAPES:
    tag = '%dx%d' % (fh, fw)
    lp = ip.get_low_pass_filter(
        (fh, fw), {'shape': 'exponential', 'cutoff': 0.3, 'order': 4.0})
    # float32-valued: the stored array compresses to half
    cx = (rs.randn(fh, fw) + 1j * rs.randn(fh, fw)).astype(
        np.complex64).astype(np.complex128)
    out['fd_lp_filter_' + tag] = lp
    out['fd_cx_filter_' + tag] = cx
    for kind, filt in (('lp', lp), ('cx', cx)):
      for i in ((0, 1) if (kind, tag) == ('lp', '37x53') else (0,)):
        name = 'fd_%s_%s_img%d' % (kind, tag, i)
        out[name] = checked(name, ip.filter_fd(img[i], filt),
                            truth_filter_fd(img[i], filt))
    if tag == '40x64':
      name = 'fd_cx_%s_u8' % tag
      out[name] = checked(name, ip.filter_fd(img_u8[0], cx),
                          truth_filter_fd(img_u8[0], cx))

  # ---- filter_sd ------------------------------------------------------------
  sd_filters = {
      '5x7': rs.randn(5, 7), '4x6': rs.randn(4, 6), '1x1': rs.randn(1, 1),
      '37x3': rs.randn(H, 3) / H}
  for tag, filt in sd_filters.items():
    out['sd_filter_' + tag] = filt
    name = 'sd_%s_img0' % tag
    out[name] = checked(name, ip.filter_sd(img[0], filt),
                        truth_filter_sd(img[0], filt))
  name = 'sd_5x7_u8'
  out[name] = checked(name, ip.filter_sd(img_u8[0], sd_filters['5x7']),
                      truth_filter_sd(img_u8[0], sd_filters['5x7']))
  vert = np.array([0.07, 0.41, 0.29, 0.17, 0.06]) * (1 + 0.1 * rs.rand(5))
  horz = np.array([0.2, 0.5, 0.3]) * (1 + 0.1 * rs.rand(3))
  out['sd_vert'], out['sd_horz'] = vert, horz
  for tag, image in (('img0', img[0]), ('u8', img_u8[0])):
    name = 'sd_separable_' + tag
    out[name] = checked(
        name, ip.filter_sd(image, None, separable_vert=vert,
                           separable_horz=horz),
        truth_filter_sd_separable(image, vert, horz))

  # ---- moves ----------------------------------------------------------------
  for f in (1, 2, 3, 5):
    out['down_%d' % f] = ip.downsample(img[0], f)
    out['down_%d_u8' % f] = ip.downsample(img_u8[0], f)
  tiles, pos = ip.patches_from_single_image(img[0], (8, 8), False)
  out['tile_8x8'] = tiles
  out['tile_8x8_positions'] = np.asarray(pos, dtype=np.int32)
  out['tile_8x8_u8'] = ip.patches_from_single_image(img_u8[0], (8, 8), True)[0]
  exact_img = rs.rand(32, 48, 1).astype(np.float32)
  out['exact_img'] = exact_img
  tiles16, pos16 = ip.patches_from_single_image(exact_img, (16, 16), True)
  out['tile_16x16'] = tiles16
  assert np.array_equal(
      ip.assemble_image_from_patches(tiles16, (16, 16), pos16), exact_img)
  perm = rs.permutation(len(pos))
  out['assemble_perm'] = perm.astype(np.int32)
  out['assemble_perm_image'] = ip.assemble_image_from_patches(
      tiles[perm], (8, 8), [pos[i] for i in perm])
  subset = np.sort(rs.choice(len(pos), len(pos) // 2, replace=False))
  out['assemble_subset'] = subset.astype(np.int32)
  out['assemble_subset_image'] = ip.assemble_image_from_patches(
      tiles[subset].reshape(len(subset), -1), (8, 8),
      [pos[i] for i in subset])
  # overlapping positions: the later patch wins
  over_pos = [(0, 0), (4, 4), (2, 9), (4, 4), (20, 30), (17, 27)]
  out['assemble_overlap_positions'] = np.asarray(over_pos, dtype=np.int32)
  out['assemble_overlap_image'] = ip.assemble_image_from_patches(
      tiles[:len(over_pos)], (8, 8), over_pos)
  out['assemble_overlap_image_u8'] = ip.assemble_image_from_patches(
      out['tile_8x8_u8'][:len(over_pos)], (8, 8), over_pos)

  # ---- unwhiten_center_surround, pSNR ----------------------------------------
  natural = zca_data.one_over_f_images(rs, 1, 96, 1)[0, :64, :48].astype(
      np.float32)
  out['natural'] = natural
  for tag, low in (('low0', 0.0), ('low1e-3', 1e-3)):
    cutoffs = {'low': low, 'high': 0.8}
    white, filt = ip.whiten_center_surround(natural, cutoffs,
                                            return_filter=True)
    assert np.abs(1. / filt).max() <= 1e3 * (1 + 1e-12)
    out['white_' + tag] = white
    name = 'unwhite_exact_' + tag
    out[name] = checked(
        name, ip.unwhiten_center_surround(white, orig_filter_DFT=filt),
        truth_filter_fd(white, 1. / filt))
    out['psnr_exact_' + tag] = np.float64(
        plotting.compute_pSNR(natural, out[name]))
  low_cutoff = 0.05
  out['low_cutoff'] = np.float64(low_cutoff)
  ramp = np.maximum(ip.get_whitening_ramp_filter((64, 48), False).real,
                    low_cutoff)
  name = 'unwhite_ramp'
  out[name] = checked(
      name, ip.unwhiten_center_surround(out['white_low0'],
                                        low_cutoff=low_cutoff),
      truth_filter_fd(out['white_low0'], 1. / ramp.astype(np.complex128)))
  out['psnr_ramp'] = np.float64(plotting.compute_pSNR(natural, out[name]))
  out['psnr_ramp_manual'] = np.float64(
      plotting.compute_pSNR(natural, out[name], manual_sig_mag=1.0))
  assert plotting.compute_pSNR(natural, natural) == np.inf

  # ---- the example's ZCA round trip with stored parameters --------------------
  zca = helpers.load('zca')
  params = {'PCA_basis': zca['n64_basis'],
            'PCA_axis_variances': zca['n64_variances'],
            'subtracted_mean': zca['n64_mean']}
  patches, positions = ip.patches_from_single_image(natural, (8, 8), True)
  white_patches = ip.whiten_ZCA(patches, params)
  out['zca_white_image'] = ip.assemble_image_from_patches(
      white_patches, (8, 8), positions)
  out['zca_recovered_image'] = ip.assemble_image_from_patches(
      ip.unwhiten_ZCA(white_patches, params), (8, 8), positions)

  path = REPO / 'tests' / 'golden' / 'image_tools.npz'
  np.savez_compressed(path, **out)
  print('wrote', path, path.stat().st_size, 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
  main()
