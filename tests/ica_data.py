"""Inputs and the float64 statement of the ICA tests (tests/golden/ica_training.npz
is written by tools/make_golden_ica.py from the same functions).

Data: independent Laplace sources mixed by a Gaussian matrix and whitened
with the float64 ZCA matrix of the mixture, drawn from
numpy.random.RandomState(seed).  Rows are samples: X = S M^T W, so the
whitened mixing matrix (the dictionary ICA should find, up to permutation
and scale, as rows) is (W M)^T."""
import numpy as np

BATCH = 250            # the batch of the reference's examples/train_ica.py
STEPSIZE = 0.1         # the example's first phase
# name -> (n, batches, seed); the fixture horizons: reference dictionaries
# after these steps
CASES = {
    'n64': (64, 40, 21),
    'n256': (256, 20, 22),
}
HORIZONS = {'n64': (1, 5, 20), 'n256': (1, 10)}
KAPPAS = (1.0, 1e2, 1e4)
CODE_ROWS = 8          # rows of each invertible_linear case kept
RECOVERY = (64, 200, 31)   # n, batches (reused every epoch), seed


def sources_and_mixing(n, count, seed):
  """(whitened data (count, n) float32, whitened mixing (n, n) float64 whose
  rows are the true basis functions)."""
  rs = np.random.RandomState(seed)
  s = rs.laplace(size=(count, n))
  mix = rs.standard_normal((n, n))
  x = s @ mix.T
  c = x.T @ x / count
  w, u = np.linalg.eigh(c)
  white = (u / np.sqrt(w)) @ u.T
  return (x @ white).astype(np.float32), (white @ mix).T


def batches(n, num_batches, seed):
  """(num_batches, BATCH, n) float32 and the whitened mixing."""
  x, mixing = sources_and_mixing(n, num_batches * BATCH, seed)
  return x.reshape(num_batches, BATCH, n), mixing


def init_dictionary(n, seed):
  """QR-orthonormal start, as examples/train_ica.py draws it."""
  q, _ = np.linalg.qr(np.random.RandomState(seed + 1000).standard_normal(
      (n, n)))
  return q.astype(np.float32)


def conditioned(n, kappa, seed):
  """(n, n) float32 matrix with singular values logspace(0, -log10 kappa)."""
  rs = np.random.RandomState(seed)
  u, _ = np.linalg.qr(rs.standard_normal((n, n)))
  v, _ = np.linalg.qr(rs.standard_normal((n, n)))
  sv = np.logspace(0, -np.log10(kappa), n)
  return ((u * sv) @ v.T).astype(np.float32)


def code_inputs(n, kappa):
  """(images (BATCH, n) float32, dictionary (n, n) float32) of an
  invertible_linear case."""
  seed = 500 + n + int(round(np.log10(kappa)))
  x, _ = sources_and_mixing(n, 4 * n, seed)   # D >= n for the whitening
  return x[:BATCH], conditioned(n, kappa, seed + 7)


def guard(x):
  """Checksum of a regenerated input: [sum, sum of squares] in float64."""
  x64 = np.asarray(x, np.float64)
  return np.array([x64.sum(), (x64 * x64).sum()])


# ---- the float64 statement of the reference's step ------------------------
def truth_step(d, x, stepsize, num_iters=1):
  """One reference iteration in float64: codes = x D^-1, then num_iters
  natural-gradient updates D += stepsize ((C^T sign C) / b - I) D."""
  c = x @ np.linalg.inv(d)
  m = c.T @ np.sign(c) / c.shape[0] - np.eye(d.shape[0])
  for _ in range(num_iters):
    d = d + stepsize * (m @ d)
  return d


def truth_run(d0, data, schedule, steps):
  """float64 run of `steps` iterations over the batches of `data`
  (schedule: iteration -> (stepsize, num_iters))."""
  d = np.asarray(d0, np.float64)
  stp = None
  for it in range(steps):
    if it in schedule:
      stp = schedule[it]
    d = truth_step(d, np.asarray(data[it % len(data)], np.float64), *stp)
  return d


def amari_index(dictionary, mixing):
  """Amari distance of G = mixing D^-1 from a scaled permutation, in [0, 1]
  (0: the sources are recovered)."""
  g = np.abs(np.asarray(mixing, np.float64) @ np.linalg.inv(
      np.asarray(dictionary, np.float64)))
  n = g.shape[0]
  rows = (g.sum(axis=1) / g.max(axis=1) - 1).sum()
  cols = (g.sum(axis=0) / g.max(axis=0) - 1).sum()
  return float((rows + cols) / (2 * n * (n - 1)))


def rel(a, b):
  a = np.asarray(a, np.float64)
  b = np.asarray(b, np.float64)
  return float(np.linalg.norm(a - b) / np.linalg.norm(b))
