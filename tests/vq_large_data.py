"""Inputs and restatement of the large-codebook vector quantiser tests
(include/vtc_vq_large.h): tests/vq_data.py as it is -- assign, step, fit,
index_counts, MARGIN and vectors are its own, the contract is the same -- plus
what the larger limit changes: the initial codebook with its cap as an
argument, the workspace formula of the header, and the Mod3 point of a scene
with more than 4096 distinct tail vectors.  Test infrastructure, like
tests/vq_data.py.
"""
import numpy as np

import quantization_data as qdata
import vq_data as base

MAX_CODEWORDS = 131072        # VTC_VQ_LARGE_MAX_CODEWORDS
SMALL_MAX_CODEWORDS = base.MAX_CODEWORDS
ROWS = base.ROWS
MARGIN = base.MARGIN
vectors, assign, step, fit, index_counts = (
    base.vectors, base.assign, base.step, base.fit, base.index_counts)


def padded(nbytes):
  return -(-nbytes // 256) * 256


def workspace_formula(b, d, kmax):
  """vtc_vq_large_lloyd_step_workspace_bytes, term by term."""
  c = -(-b // ROWS)
  return (padded(4 * b) + padded(8 * b) +
          padded(4 * ROWS * c) + padded(4 * c) + padded(8 * ROWS * c * d) +
          padded(8 * ROWS * c) + padded(4 * ROWS * c) +
          padded(8 * kmax) + padded(8 * kmax) + padded(8 * kmax) +
          padded(4 * kmax) + 256 + 256)


def initial_codebook(x, num_bins, max_codewords=SMALL_MAX_CODEWORDS):
  """vq_data.initial_codebook with the cap as an argument: the rows
  floor(i * b / m), m = min(num_bins, b, max_codewords), without those that
  hold a NaN, behind the zero vector; bitwise duplicates removed (the first
  stays, -0.0 is 0.0); at most max_codewords rows.  float64 (k, d)."""
  b, d = x.shape
  m = min(int(num_bins), b, int(max_codewords))
  rows, seen = [], set()
  for row in [np.zeros(d, np.float32)] + [x[(i * b) // m] for i in range(m)]:
    if np.isnan(row).any():
      continue
    row = np.where(row == 0, np.float32(0.0), row).astype(np.float32)
    key = row.tobytes()
    if key not in seen:
      seen.add(key)
      rows.append(row)
  return np.array(rows[:int(max_codewords)], dtype=np.float64)


def steps(x, book, lam, epsilon, pin_zero, count):
  """The states after 0 .. count steps from the codebook `book` (kmax = its
  rows), and the smallest margin of every assignment made on the way."""
  state, margin = base.initial_state(x, book)
  states = [state]
  for _ in range(count):
    state, facts = base.step(x, state, lam, epsilon, pin_zero)
    margin = min(margin, facts['margin'])
    states.append(state)
  return states, margin


# ------------------------------------------------------------ the R-D scene
RD_ROWS = 5632          # 176 copies of the 32 patches of vq_data.scene()
RD_SEED = 61
RD_ITERATIONS, RD_EPSILON = 2, 1e-3
RD_SCAL_MULT, RD_VEC_MULT = 2.0, 30.0


def scene():
  """vq_data.scene() tiled to RD_ROWS rows, seeded noise on every code and
  patch, and the tail of every fourth row exactly zero: three quarters of the
  rows have a tail of their own, so that vec_init_num_bins = 100000 finds more
  than 4096 distinct candidates, and the zero cell is large and cheap enough
  for a Lagrange multiplier of RD_VEC_MULT to pull other rows into it (a start
  in which every row is its own codeword, all of one length, would be a fixed
  point)."""
  s = base.scene()
  rs = np.random.RandomState(RD_SEED)
  copies = RD_ROWS // len(s['codes'])
  codes = np.tile(s['codes'], (copies, 1)).astype(np.float64)
  codes += rs.laplace(size=codes.shape) * 3.0
  codes[::4, base.VEC_CLUST] = 0.0
  patches = np.tile(s['patches'], (copies, 1)).astype(np.float64)
  patches += rs.randn(*patches.shape)
  return {'patches': patches.astype(np.float32),
          'dictionary': s['dictionary'], 'codes': codes.astype(np.float32)}


def mod3_point(s, max_codewords):
  """The training call of Mod3_compute_RD_point(vec_init_num_bins=100000,
  vec_max_codewords=max_codewords) on the scene: vq_data.rd_point with the
  cap as an argument."""
  scal_codes = s['codes'][:, base.SCAL_CLUSTS]
  scal, history, first = qdata.fit(
      scal_codes, *base.uniform_codebooks(scal_codes, base.SCAL_WIDTH),
      RD_SCAL_MULT, RD_ITERATIONS, RD_EPSILON, True)
  margins = [first] + [facts['margin'] for facts in history]
  vec_x = s['codes'][:, base.VEC_CLUST]
  vec, history, first = base.fit(
      vec_x, initial_codebook(vec_x, 100000, max_codewords), RD_VEC_MULT,
      RD_ITERATIONS, RD_EPSILON, True)
  margins += [first] + [facts['margin'] for facts in history]
  point = base.mixed_point(s, scal['codebooks'], scal['k'], scal['lengths'],
                           RD_SCAL_MULT, vec, RD_VEC_MULT)
  point['margin'] = min([point['margin']] + margins)
  point.update(vec=vec, scal=scal)
  return point
