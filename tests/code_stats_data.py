"""Seeded builders of the inputs of the code-statistics tests, so that
tests/golden/code_stats.npz stores expected outputs only
(tools/make_code_stats_golden.py writes it from these same arrays)."""
import numpy as np

ROWS, COLS = 4099, 70          # no multiple of any block of rows; two tiles
LATTICE = (10, 11, 12)         # multiples of 0.1, 0.25, 0.1: dequantised codes
CONSTANT, ALL_ZERO, LAST_ONLY = 20, 30, 40
BINS = (1, 7, 100, 1000)
# name -> (ignore_vals, overlaid)
VARIANTS = {'zero': ([0.0], False), 'none': ([], False),
            'overlaid': ([0.0], True)}
PAIRS = ((0, 1), (5, 5), (69, 0), (10, 11), (30, 1))   # the last one is empty
JOINT_BINS = (1, 16, 64, 256)
# name -> (h, w, nbins, centred coordinates)
ROTATIONAL = {'16x16': (16, 16, 10, False), '17x9': (17, 9, 4, False),
              'centred': (16, 16, 10, True), 'empty': (5, 5, 12, False)}
STACK = 3


def marginal_codes():
  """(4099, 70) float32: about 70 % exact zeros, the rest Laplacian; three
  columns on a lattice, the way utils.jpeg.dequantize makes them (float64
  level * width, rounded to float32); one constant column (lo == hi), one
  all-zero column (nothing kept under ignore_vals = [0.0]) and one whose only
  non-zero is its last row."""
  rs = np.random.RandomState(20261)
  x = rs.laplace(scale=1.0, size=(ROWS, COLS))
  for col, width, most in zip(LATTICE, (0.1, 0.25, 0.1), (32, 28, 16)):
    x[:, col] = rs.randint(-most, most + 1, size=ROWS).astype(np.float64) * width
  x = x.astype(np.float32)
  x[rs.rand(ROWS, COLS) < 0.7] = 0.0
  x[:, CONSTANT] = 1.5
  x[:, ALL_ZERO] = 0.0
  x[:, LAST_ONLY] = 0.0
  x[-1, LAST_ONLY] = -2.25
  return x


def kept_values(column, ignore_vals):
  """The reference's filter_code_vals on one column."""
  keep = np.ones(len(column), dtype=bool)
  for v in ignore_vals:
    keep &= column != np.float32(v)
  return column[keep]


def float64_edges(lo, hi, bins):
  """The contract's edges: np.linspace in float64 whatever numpy is here."""
  return np.linspace(np.float64(lo), np.float64(hi), bins + 1)


def floor_formula_bins(values, lo, hi, bins):
  """The uncorrected guess floor((x - lo) * bins / (hi - lo)) in float64,
  the right edge folded into the last bin: what a histogram without the
  comparison against the edges would count."""
  x = values.astype(np.float64)
  k = np.floor((x - lo) * bins / (hi - lo)).astype(np.int64)
  return np.bincount(np.clip(k, 0, bins - 1), minlength=bins)


def rotational_inputs(name):
  """(stack float64 (3, h, w), coordinates or None) of one ROTATIONAL case."""
  h, w, _, centred = ROTATIONAL[name]
  rs = np.random.RandomState(sorted(ROTATIONAL).index(name) + 77)
  stack = rs.randn(STACK, h, w) + 3.0
  coords = None
  if centred:
    coords = tuple(np.meshgrid(np.arange(h) - h // 2, np.arange(w) - w // 2,
                               indexing='ij'))
  return stack, coords
