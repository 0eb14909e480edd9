"""Float64 numpy restatement of the reference's compute_ssim
(utils/plotting.py:42-64), i.e. of scikit-image's compare_ssim(target,
reconstruction, data_range=R, gaussian_weights=True, sigma=1.5,
use_sample_covariance=False) for 2-d images, for the SSIM tests.  numpy only:
the GPU machines have neither scipy nor the reference.

The window is scipy.ndimage.gaussian_filter's: 11 taps per axis,
exp(-k^2 / (2 * 1.5^2)) for k = -5 .. 5 over their sum, the vertical axis
first, then the horizontal one, boundary 'reflect' (the edge sample repeated).
Here it is a plain tap sum in ascending tap order over indices folded with
period 2n, the rule of csrc/sep_filter.h.  tests/test_ssim_host.py holds this
file to tests/golden/ssim.npz, which tools/make_ssim_golden.py wrote with
scipy itself.
"""
import numpy as np

SIGMA = 1.5
RADIUS = 5          # int(3.5 * 1.5 + 0.5)
TAPS = 2 * RADIUS + 1
K1, K2 = 0.01, 0.03


def fold(i, n):
  """numpy's 'symmetric' padding as an index map: period 2n, the second half
  mirrored.  Right for windows wider than the axis."""
  m = np.mod(i, 2 * n)
  return np.where(m < n, m, 2 * n - 1 - m)


def gaussian_taps():
  k = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
  g = np.exp(-0.5 / (SIGMA * SIGMA) * k ** 2)
  return g / g.sum()


def filter_axis(a, axis):
  a = np.asarray(a, dtype=np.float64)
  n = a.shape[axis]
  taps = gaussian_taps()
  out = np.zeros(a.shape, dtype=np.float64)
  for k in range(TAPS):
    out = out + np.take(a, fold(np.arange(n) + k - RADIUS, n), axis) * taps[k]
  return out


def window(a):
  return filter_axis(filter_axis(a, 0), 1)


def derived_range(target):
  """R for manual_sig_mag=None: max - min in the target's own precision (a
  float32 difference for a float32 target), widened to float64."""
  target = np.asarray(target)
  return float(target.max() - target.min())


def ssim(target, reconstruction, data_range=None):
  """(mean of the cropped map, the whole map), both float64."""
  if data_range is None:
    data_range = derived_range(target)
  x = np.asarray(target).astype(np.float64)
  y = np.asarray(reconstruction).astype(np.float64)
  if x.ndim != 2 or x.shape != y.shape:
    raise ValueError('two 2-d images of one shape')
  if min(x.shape) < TAPS:
    raise ValueError('win_size exceeds image extent')
  r = float(data_range)
  ux, uy = window(x), window(y)
  uxx, uyy, uxy = window(x * x), window(y * y), window(x * y)
  vx = uxx - ux * ux
  vy = uyy - uy * uy
  vxy = uxy - ux * uy
  c1, c2 = (K1 * r) ** 2, (K2 * r) ** 2
  a1, a2 = 2 * ux * uy + c1, 2 * vxy + c2
  b1, b2 = ux ** 2 + uy ** 2 + c1, vx + vy + c2
  s = (a1 * a2) / (b1 * b2)
  return float(s[RADIUS:-RADIUS, RADIUS:-RADIUS].mean(dtype=np.float64)), s
