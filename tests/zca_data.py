"""Inputs and the float64 statement of the ZCA / PCA tests (tests/golden/zca.npz
is written by tools/make_golden_zca.py from the same functions).

Inputs: patches of synthetic 1/f-spectrum images, each image range-standardised
to [0, 1] (mean ~0.5, spread ~0.1: the cancellation case of an uncentred
covariance), drawn from numpy.random.RandomState(seed)."""
import numpy as np

EPS = 1e-4
# name -> (n, patch (h, w, c), estimation rows D, held-out rows, seed)
CASES = {
    'n64': (64, (8, 8, 1), 4096, 512, 11),
    'n192': (192, (8, 8, 3), 4096, 512, 12),
    'n256': (256, (16, 16, 1), 4096, 512, 13),
}
IMAGES, IMAGE_SIZE = 8, 96
STORED_ROWS = 16   # rows of each reference output kept in the fixture


def one_over_f_images(rs, count, size, channels):
  noise = rs.randn(count, size, size, channels)
  fy = np.fft.fftfreq(size)[:, None]
  fx = np.fft.fftfreq(size)[None, :]
  f = np.sqrt(fy * fy + fx * fx)
  f[0, 0] = 1.0 / size
  spec = np.fft.fft2(noise, axes=(1, 2)) / f[None, :, :, None]
  img = np.real(np.fft.ifft2(spec, axes=(1, 2)))
  lo = img.min(axis=(1, 2, 3), keepdims=True)
  hi = img.max(axis=(1, 2, 3), keepdims=True)
  return (img - lo) / (hi - lo)


def draw_patches(rs, images, count, ph, pw):
  num, h, w, c = images.shape
  out = np.empty((count, ph * pw * c), dtype=np.float32)
  idx = rs.randint(0, num, size=count)
  vert = rs.randint(0, h - ph + 1, size=count)
  horz = rs.randint(0, w - pw + 1, size=count)
  for p in range(count):
    out[p] = images[idx[p], vert[p]:vert[p] + ph,
                    horz[p]:horz[p] + pw, :].reshape(-1)
  return out


def case_data(name):
  """(estimation patches (D, n), held-out patches (D_test, n)), float32."""
  n, (ph, pw, c), d_est, d_test, seed = CASES[name]
  rs = np.random.RandomState(seed)
  images = one_over_f_images(rs, IMAGES, IMAGE_SIZE, c)
  est = draw_patches(rs, images, d_est, ph, pw)
  held = draw_patches(rs, images, d_test, ph, pw)
  assert est.shape[1] == n
  return est, held


def pca_data():
  """Mean-zero (4096, 64) float32 data for training.pca.train_dictionary."""
  est, _ = case_data('n64')
  return (est - est.mean(axis=0, dtype=np.float64)).astype(np.float32)


def guard(x):
  """Checksum of a regenerated input: [sum, sum of squares] in float64."""
  x64 = x.astype(np.float64)
  return np.array([x64.sum(), (x64 * x64).sum()])


# ---- the float64 statement of the reference's formulas -------------------
def eigh_desc(c):
  w, u = np.linalg.eigh(c)
  return w[::-1], u[:, ::-1]


def truth_estimate(x):
  """whiten_ZCA(x) without parameters, in float64: per-component centring,
  covariance / D, W = U diag(1/(sqrt(w)+eps)) U^T, + mean of the means."""
  x64 = x.astype(np.float64)
  mu = x64.mean(axis=0)
  xc = x64 - mu
  w, u = eigh_desc(xc.T @ xc / x.shape[0])
  m = mu.mean()
  wm = (u / (np.sqrt(np.maximum(w, 0)) + EPS)) @ u.T
  return xc @ wm + m, {'PCA_basis': u, 'PCA_axis_variances': w,
                       'subtracted_mean': m}


def truth_whiten(x, params):
  """whiten_ZCA(x, params) in float64: the scalar mean is subtracted."""
  u = np.asarray(params['PCA_basis'], np.float64)
  w = np.asarray(params['PCA_axis_variances'], np.float64)
  m = float(params['subtracted_mean'])
  wm = (u / (np.sqrt(np.maximum(w, 0)) + EPS)) @ u.T
  return (x.astype(np.float64) - m) @ wm + m


def truth_unwhiten(x, params):
  u = np.asarray(params['PCA_basis'], np.float64)
  w = np.asarray(params['PCA_axis_variances'], np.float64)
  m = float(params['subtracted_mean'])
  wi = (u * (np.sqrt(np.maximum(w, 0)) + EPS)) @ u.T
  return (x.astype(np.float64) - m) @ wi + m


def rel(a, b):
  a = np.asarray(a, np.float64)
  b = np.asarray(b, np.float64)
  return float(np.linalg.norm(a - b) / np.linalg.norm(b))
