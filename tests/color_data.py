"""The truth of the colour tests (include/ext/vtc_color.h, utils/color.py),
restated from the header in numpy float64: the 3 x 3 affine map per pixel in
either layout, the box mean, the replicate and triangle upsamplers, the JFIF
constants, ITU-T T.81 Annex K.2 and its zig-zag, and the images and the DCT
basis the GPU tests share.  The header fixes the order of every operation and
numpy rounds every float64 operation on its own, so the comparisons are
between float32 bit patterns.  No GPU and no product code."""
import functools

import numpy as np

HWC, CHW = 0, 1                     # VTC_COLOR_HWC, VTC_COLOR_CHW
REPLICATE, TRIANGLE = 0, 1          # VTC_UPSAMPLE_*
FACTORS = (1, 2, 4)

# JFIF 1.02: the ten decimal constants
FORWARD = np.array([[0.299, 0.587, 0.114],
                    [-0.168736, -0.331264, 0.5],
                    [0.5, -0.418688, -0.081312]])
INVERSE = np.array([[1.0, 0.0, 1.402],
                    [1.0, -0.344136, -0.714136],
                    [1.0, 1.772, 0.0]])

# ITU-T T.81 Annex K.2, the chrominance quantisation table
ANNEX_K2 = np.array([[17, 18, 24, 47, 99, 99, 99, 99],
                     [18, 21, 26, 66, 99, 99, 99, 99],
                     [24, 26, 56, 99, 99, 99, 99, 99],
                     [47, 66, 99, 99, 99, 99, 99, 99],
                     [99, 99, 99, 99, 99, 99, 99, 99],
                     [99, 99, 99, 99, 99, 99, 99, 99],
                     [99, 99, 99, 99, 99, 99, 99, 99],
                     [99, 99, 99, 99, 99, 99, 99, 99]])


def bits(a):
  """The bit patterns of a float32 array; NaNs compare by their class (every
  NaN is one pattern), everything else bit for bit (-0.0 is not 0.0)."""
  a = np.ascontiguousarray(a, dtype=np.float32)
  out = a.view(np.uint32).copy()
  out[np.isnan(a)] = 0x7fc00000
  return out


def same_bits(a, b):
  a, b = np.asarray(a), np.asarray(b)
  return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _f32(v):
  with np.errstate(over='ignore', invalid='ignore'):
    return v.astype(np.float32)


# ------------------------------------------------------------ the affine map
def color_transform(x, matrix, pre=None, post=None, clamp=None, layout=HWC,
                    out_layout=None):
  """x float32 (count, h, w, 3) or (count, 3, h, w) -> float32 in out_layout.
  t_j = x_j - pre_j; out_i = ((m_i0 t_0 + m_i1 t_1) + m_i2 t_2) + post_i; then
  v < lo ? lo : (v > hi ? hi : v)."""
  out_layout = layout if out_layout is None else out_layout
  m = np.asarray(matrix, dtype=np.float64).reshape(3, 3)
  pre = np.zeros(3) if pre is None else np.asarray(pre, dtype=np.float64)
  post = np.zeros(3) if post is None else np.asarray(post, dtype=np.float64)
  x = np.asarray(x, dtype=np.float32)
  assert x.ndim == 4 and x.shape[3 if layout == HWC else 1] == 3
  axis = 3 if layout == HWC else 1
  with np.errstate(over='ignore', invalid='ignore'):
    t = [np.take(x, j, axis=axis).astype(np.float64) - pre[j]
         for j in range(3)]
    planes = []
    for i in range(3):
      v = ((m[i, 0] * t[0] + m[i, 1] * t[1]) + m[i, 2] * t[2]) + post[i]
      if clamp is not None:
        lo, hi = float(clamp[0]), float(clamp[1])
        v = np.where(v < lo, lo, np.where(v > hi, hi, v))
      planes.append(_f32(v))
  return np.stack(planes, axis=3 if out_layout == HWC else 1)


def rgb_to_ycbcr(x, offset=128.0, **kw):
  return color_transform(x, FORWARD, post=(0.0, offset, offset), **kw)


def ycbcr_to_rgb(x, offset=128.0, clamp=None, **kw):
  return color_transform(x, INVERSE, pre=(0.0, offset, offset), clamp=clamp,
                         **kw)


# -------------------------------------------------------------- resampling
def ceil_div(a, b):
  return -(-a // b)


def downsample(planes, fv, fh):
  """(count, h, w) -> (count, ceil(h / fv), ceil(w / fh)): the sum from 0.0 in
  row-major order of the pixels of the box that exist, over their number."""
  x = np.asarray(planes, dtype=np.float32).astype(np.float64)
  count, h, w = x.shape
  total = np.zeros((count, ceil_div(h, fv), ceil_div(w, fh)))
  number = np.zeros(total.shape[1:])
  for dy in range(fv):
    for dx in range(fh):
      part = x[:, dy::fv, dx::fh]
      total[:, :part.shape[1], :part.shape[2]] += part
      number[:part.shape[1], :part.shape[2]] += 1.0
  with np.errstate(invalid='ignore'):
    return _f32(total / number)


def taps(n_out, f, n_in):
  """(a, b, t) of every output index of one axis."""
  u = (np.arange(n_out, dtype=np.float64) + 0.5) / float(f) - 0.5
  i0 = np.floor(u)
  t = u - i0
  i0 = i0.astype(np.int64)
  return (np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), t)


def upsample(planes, fv, fh, shape, mode):
  """(count, h_in, w_in) -> (count, h_out, w_out), shape = (h_out, w_out)."""
  x = np.asarray(planes, dtype=np.float32)
  h_out, w_out = shape
  count, h_in, w_in = x.shape
  assert ceil_div(h_out, fv) == h_in and ceil_div(w_out, fh) == w_in
  if mode == REPLICATE:
    return x[:, np.arange(h_out) // fv][:, :, np.arange(w_out) // fh].copy()
  p = x.astype(np.float64)
  av, bv, tv = taps(h_out, fv, h_in)
  ah, bh, th = taps(w_out, fh, w_in)
  tv = tv[None, :, None]
  th = th[None, None, :]
  with np.errstate(invalid='ignore'):
    top = (1.0 - th) * p[:, av][:, :, ah] + th * p[:, av][:, :, bh]
    bottom = (1.0 - th) * p[:, bv][:, :, ah] + th * p[:, bv][:, :, bh]
    return _f32((1.0 - tv) * top + tv * bottom)


# ------------------------------------------------------------------ tables
def zigzag_positions(n=8):
  """ITU-T T.81 figure A.6: the anti-diagonals in turn, even ones upwards."""
  out = []
  for s in range(2 * n - 1):
    cells = [(v, s - v) for v in range(n) if 0 <= s - v < n]
    out += cells[::-1] if s % 2 == 0 else cells
  return out


def chroma_binwidths():
  return np.array([ANNEX_K2[v, h] for v, h in zigzag_positions()],
                  dtype=np.float64)


def scan_order(n=8):
  return np.array([v * n + h for v, h in zigzag_positions(n)], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def dct_basis(p=8):
  """(p p, p p) float32, row p u + v the DCT-II basis image (u, v) flattened
  row-major; orthonormal."""
  k = np.arange(p)
  one_d = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / (2 * p))
  one_d *= np.where(k == 0, np.sqrt(1. / p), np.sqrt(2. / p))[:, None]
  basis = np.einsum('ui,vj->uvij', one_d, one_d).reshape(p * p, p * p)
  assert np.abs(basis @ basis.T - np.eye(p * p)).max() < 1e-12
  return basis.astype(np.float32)


# ------------------------------------------------------------------ inputs
def colour_image(h, w, seed=3347):
  """(h, w, 3) float32 in [0, 255]: smooth plus noise, the channels
  different."""
  rs = np.random.RandomState(seed)
  yy, xx = np.mgrid[0:h, 0:w]
  planes = []
  for c, (a, b, d) in enumerate(((5., 7., 11.), (6., 9., 13.), (4., 8., 10.))):
    smooth = (np.sin(yy / a + c) + np.cos(xx / b) + np.sin((yy + xx) / d)) / 3.
    planes.append(127.5 + (100. - 15. * c) * smooth + 6. * rs.randn(h, w))
  return np.clip(np.stack(planes, axis=2), 0., 255.).astype(np.float32)


def wild_stack(count, h, w, layout=HWC, seed=0):
  """A float32 stack with values below 0 and above 255 and, where there is
  room, one NaN, one +inf and one -inf."""
  rs = np.random.RandomState(1000 * seed + 97 * count + 13 * h + w)
  x = (rs.rand(count, h, w, 3) * 400. - 70.).astype(np.float32)
  flat = x.reshape(-1)
  if flat.size >= 48:
    flat[7], flat[flat.size // 2], flat[flat.size - 5] = (np.nan, np.inf,
                                                          -np.inf)
  return x if layout == HWC else np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def plane_stack(count, h, w, seed=0):
  rs = np.random.RandomState(2000 * seed + 89 * count + 17 * h + w)
  return (rs.rand(count, h, w) * 300. - 20.).astype(np.float32)


def colours_8bit(n=4096, seed=11):
  """(1, 1, n, 3) float32: n random 8-bit colours, the corners of the cube and
  the greys 0 and 255 among them."""
  rs = np.random.RandomState(seed)
  x = rs.randint(0, 256, size=(n, 3))
  corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255)
                      for b in (0, 255)])
  x[:8] = corners
  return x.astype(np.float32).reshape(1, 1, n, 3)


DENSE = np.array([[0.31, -1.7, 0.055], [2.25, 0.4, -0.93],
                  [-0.6, 0.128, 1.01]])
DENSE_PRE = (3.5, -20.25, 100.1)
DENSE_POST = (-7.75, 0.3, 64.0)
