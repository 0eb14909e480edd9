"""The three-part bf16 split of csrc/split_operand.h (split3_packed), restated
in numpy: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), round to nearest
even.  The parts sum to x exactly, and the six part products the kernels keep
(hh, hm, mh, hl, lh, mm) leave the gradient at the rounding of E."""
import numpy as np

KEPT = [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)]


def bf16_rne(x):
  """float32 -> nearest bfloat16 (ties to even), returned as float32."""
  bits = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
  bits = (bits + 0x7fff + ((bits >> 16) & 1)) & 0xffff0000
  return bits.astype(np.uint32).view(np.float32)


def split3(x):
  x = np.asarray(x, dtype=np.float32)
  h = bf16_rne(x)
  r1 = x - h
  m = bf16_rne(r1)
  l = bf16_rne(r1 - m)
  return h, m, l


def _assert_exact(x):
  h, m, l = split3(x)
  total = h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64)
  assert (total == x.astype(np.float64)).all()
  for part in (h, m, l):                   # each part is a bfloat16
    assert (part.view(np.uint32) & 0xffff == 0).all()


def test_parts_sum_to_the_value_on_random_floats():
  rs = np.random.RandomState(0)
  _assert_exact(rs.randn(1 << 16).astype(np.float32))
  _assert_exact((0.05 * rs.randn(1 << 16) * (rs.rand(1 << 16) < 0.2)).astype(
      np.float32))
  # random bit patterns with exponents well inside the normal range
  bits = rs.randint(0, 1 << 23, 1 << 16).astype(np.uint32)
  bits |= rs.randint(64, 192, 1 << 16).astype(np.uint32) << 23
  bits |= rs.randint(0, 2, 1 << 16).astype(np.uint32) << 31
  _assert_exact(bits.view(np.float32))


def test_parts_sum_to_the_value_with_all_24_bits_set():
  x = np.ldexp(np.float32(2 ** 24 - 1), np.arange(-60, 40)).astype(np.float32)
  _assert_exact(x)
  _assert_exact(-x)
  # 0x955555: a value that needs all three parts
  y = np.ldexp(np.float32(0x955555), np.arange(-60, 40)).astype(np.float32)
  _assert_exact(y)
  assert all((part != 0).all() for part in split3(y))


def test_powers_of_two_are_the_first_part_alone():
  x = np.ldexp(np.float32(1), np.arange(-100, 100)).astype(np.float32)
  h, m, l = split3(x)
  assert (h == x).all() and (m == 0).all() and (l == 0).all()


def _kept_products(a_parts, b_parts):
  """sum of the kept part products, each exact, summed in float64"""
  return sum(a_parts[p].astype(np.float64) @ b_parts[q].astype(np.float64)
             for p, q in KEPT)


def test_truncation_floor_of_the_six_product_gradient():
  """G = C^T (C D - X) from the six kept products, E rounded to float32 as the
  workspace holds it: the rounding of E dominates (2e-8 at (4096, 256, 1024);
  a two-part split with three products gives 4e-6)."""
  b, n, s = 512, 64, 128
  rs = np.random.RandomState(100 + n)
  X = (0.1 * rs.randn(b, n)).astype(np.float32)
  D = rs.randn(s, n).astype(np.float32)
  D /= np.linalg.norm(D, axis=1, keepdims=True).astype(np.float32)
  C = (0.05 * rs.randn(b, s) * (rs.rand(b, s) < 0.2)).astype(np.float32)
  c_parts = split3(C)
  E = (_kept_products(c_parts, split3(D)) - X.astype(np.float64)).astype(
      np.float32)
  G = _kept_products([p.T for p in c_parts], split3(E))
  C64, D64, X64 = (a.astype(np.float64) for a in (C, D, X))
  ref = C64.T @ (C64 @ D64 - X64)
  err = np.linalg.norm(G - ref) / np.linalg.norm(ref)
  print('six kept products, E in float32: %.3e' % err)
  assert err < 1e-7
