"""
Writes tests/golden/ssim.npz: seeded image pairs and the SSIM the reference's
compute_ssim (utils/plotting.py:42-64) gives for them.

The reference calls skimage.measure.compare_ssim(target, reconstruction,
data_range=R, gaussian_weights=True, sigma=1.5, use_sample_covariance=False).
scikit-image is not installed where this project is developed or tested, so
that function cannot be called; what stands in for it is its own recipe for
2-d images, restated below on scipy.ndimage.gaussian_filter(sigma=1.5,
truncate=3.5, mode='reflect'), the one library call scikit-image makes: five
filtered planes in float64, the SSIM formula with C1 = (0.01 R)^2 and
C2 = (0.03 R)^2, the mean over the map cropped by 5 samples per side.

Shapes: 11x11 (one cropped sample, every tap reflected on both sides), 12x17,
16x32 (exactly one tile of csrc/ssim.hip), 17x33 (one tile plus one sample in
each axis), 37x131 (ragged, several blocks), 11x300 and 300x11 (one axis all
halo).  Data: range 1, range 255, zero-centred (ux * uy can be negative), and
a constant image with one outlier pixel against the same image with the
outlier elsewhere (the cancellation case).  All float32.

Per pair `<kind>_<h>x<w>_`: x, y, range (the R given), map and mean for it,
range_none (the float32 max - min of x, widened) and mean_none for it.  Every
sample of both images lies within +-2 R for either R: the condition under
which the tests' 1e-9 bound is derived; asserted here.

Deterministic.  Needs scipy; the tests do not (tests/ssim_oracle.py).

  python tools/make_ssim_golden.py
"""
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'tests'))
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import scipy  # noqa: E402
import scipy.ndimage  # noqa: E402

import ssim_oracle  # noqa: E402

SHAPES = [(11, 11), (12, 17), (16, 32), (17, 33), (37, 131), (11, 300),
          (300, 11)]
KINDS = ['range1', 'range255', 'centred', 'outlier']
HELPER_BOUND = 1e-11


def make_pair(kind, h, w):
  """(x, y, R): float32 images and the range handed to compute_ssim."""
  rs = np.random.RandomState(1000 * KINDS.index(kind) + 7 * h + w)
  if kind == 'range1':
    x = rs.rand(h, w)
    y = np.clip(x + 0.1 * rs.randn(h, w), 0., 1.)
    r = 1.0
  elif kind == 'range255':
    x = 255. * rs.rand(h, w)
    y = np.clip(x + 20. * rs.randn(h, w), 0., 255.)
    r = 255.0
  elif kind == 'centred':
    x = np.clip(0.5 * rs.randn(h, w), -2., 2.)
    y = np.clip(x + 0.3 * rs.randn(h, w), -2., 2.)
    r = 1.0
  else:
    x = np.full((h, w), 0.5)
    y = np.full((h, w), 0.5)
    at = (int(rs.randint(h)), int(rs.randint(w)))
    to = ((at[0] + 1 + int(rs.randint(h - 1))) % h, (at[1] + 3) % w)
    assert at != to
    x[at] = 1.5
    y[to] = 1.5
    r = 1.0
  return x.astype(np.float32), y.astype(np.float32), r


def scipy_ssim(x, y, r):
  """scikit-image's structural_similarity for 2-d inputs with the reference's
  arguments, on scipy's filter."""
  x, y = x.astype(np.float64), y.astype(np.float64)

  def window(a):
    return scipy.ndimage.gaussian_filter(a, sigma=1.5, truncate=3.5,
                                         mode='reflect')
  ux, uy = window(x), window(y)
  uxx, uyy, uxy = window(x * x), window(y * y), window(x * y)
  cov_norm = 1.0   # use_sample_covariance=False
  vx = cov_norm * (uxx - ux * ux)
  vy = cov_norm * (uyy - uy * uy)
  vxy = cov_norm * (uxy - ux * uy)
  c1, c2 = (0.01 * r) ** 2, (0.03 * r) ** 2
  a1, a2, b1, b2 = (2 * ux * uy + c1, 2 * vxy + c2, ux ** 2 + uy ** 2 + c1,
                    vx + vy + c2)
  s = (a1 * a2) / (b1 * b2)
  pad = 5   # (win_size - 1) // 2, win_size = 11
  return float(s[pad:-pad, pad:-pad].mean(dtype=np.float64)), s


def main():
  out = {'scipy_version': np.array(scipy.__version__),
         'cases': np.array(['%s_%dx%d' % (kind, h, w)
                            for kind in KINDS for h, w in SHAPES])}
  worst = 0.0
  for kind in KINDS:
    for h, w in SHAPES:
      x, y, r = make_pair(kind, h, w)
      r_none = float(x.max() - x.min())   # float32 difference
      assert x.dtype == np.float32 and r_none > 0
      for bound in (r, r_none):
        assert max(np.abs(x).max(), np.abs(y).max()) <= 2 * bound, (kind, h, w)
      mean, smap = scipy_ssim(x, y, r)
      mean_none, smap_none = scipy_ssim(x, y, r_none)
      for want_mean, want_map, given in ((mean, smap, r),
                                         (mean_none, smap_none, None)):
        got_mean, got_map = ssim_oracle.ssim(x, y, given)
        gap = max(abs(got_mean - want_mean),
                  float(np.abs(got_map - want_map).max()))
        worst = max(worst, gap)
        assert gap < HELPER_BOUND, (kind, h, w, gap)
      tag = '%s_%dx%d_' % (kind, h, w)
      out.update({tag + 'x': x, tag + 'y': y, tag + 'range': np.float64(r),
                  tag + 'map': smap, tag + 'mean': np.float64(mean),
                  tag + 'range_none': np.float64(r_none),
                  tag + 'mean_none': np.float64(mean_none)})
  path = REPO / 'tests' / 'golden' / 'ssim.npz'
  np.savez_compressed(path, **out)
  print('wrote %s: %d pairs, %d bytes, scipy %s, numpy restatement within '
        '%.1e' % (path, len(out['cases']), path.stat().st_size,
                  scipy.__version__, worst))
  assert path.stat().st_size < (1 << 20)


if __name__ == '__main__':
  main()
