"""Seeded inputs of the vector quantisation tests and the float64 numpy
restatement of the contract of include/vtc_vq.h: assign, one Lloyd step, a
fit, the initial codebook, and the Mod2 / Mod3 composition of
utils.vector_quantization on top of tests/quantization_data.py.  The reference
has no utils.quantization to compare against, so this restatement is the truth
of tests/golden/vq.npz (tools/make_vq_golden.py) and of the GPU tests.  It is
test infrastructure, like tests/quantization_data.py.

A quantiser state is a dict of numpy arrays: codebook float64 (kmax, d),
lengths float64 [kmax], counts int64 [kmax], cost float64 [3], k, zero_index,
active, iterations int32 [1].  Slots past k are never read; a step writes 0.0,
0.0, 0 there.
"""
import numpy as np

import quantization_data as qdata

MAX_DIM = 32              # VTC_VQ_MAX_DIM
MAX_CODEWORDS = 4096      # VTC_VQ_MAX_CODEWORDS
ASSIGN_ROWS = 256         # VTC_VQ_ASSIGN_ROWS
TILE_DOUBLES = 4096       # VTC_VQ_TILE_DOUBLES
ROWS = 2048               # VTC_VQ_ROWS
MARGIN = qdata.MARGIN     # second-best cost - best > MARGIN * (1 + best)

STATE_FLOAT = ('codebook', 'lengths', 'cost')
STATE_INT = ('counts', 'k', 'zero_index', 'active', 'iterations')


def tile_codewords(d):
  """Whole codewords of one LDS tile of the scan (include/vtc_vq.h)."""
  return TILE_DOUBLES // min(dp for dp in (4, 8, 16, 24, 32) if d <= dp)


# --------------------------------------------------------------------- inputs
def vectors(seed, b, d, zero_rows=0.6, zeros=0.75, scale=0.7):
  """Laplace vectors; a share `zero_rows` of the rows is the zero vector, a
  share `zeros` of the other elements exactly 0.0 (0.6 + 0.4 * 0.75 = 90 % of
  all elements); float32."""
  rs = np.random.RandomState(seed)
  x = rs.laplace(size=(b, d)) * scale
  x[rs.rand(b, d) < zeros] = 0.0
  x[rs.rand(b) < zero_rows] = 0.0
  return x.astype(np.float32)


def random_codebook(seed, k, d, scale=2.0):
  """k codewords, the first the zero vector; float64 (k, d)."""
  book = np.random.RandomState(seed).laplace(size=(k, d)) * scale
  book[0] = 0.0
  return book


# name -> (seed, b, d, num_bins, lambda, max_iterations, epsilon, pin_zero)
FITS = {
    'one':         (21, 1, 1, 1, 0.0, 3, 1e-3, True),
    'pairs':       (22, 65, 2, 16, 0.0, 12, 1e-3, True),
    'sparse':      (23, 2 * ROWS + 3, 23, 500, 0.0, 6, 1e-3, True),
    'sparse_ec':   (24, 2 * ROWS + 3, 23, 500, 0.5, 6, 1e-3, True),
    'sparse_free': (25, 2 * ROWS + 3, 23, 500, 0.0, 4, 1e-3, False),
    'sparse_ec_free': (26, 2 * ROWS + 3, 23, 500, 0.5, 4, 1e-3, False),
}
SPARSE = tuple(name for name in sorted(FITS) if name.startswith('sparse'))


def fit_inputs(name):
  seed, b, d, num_bins = FITS[name][:4]
  x = vectors(seed, b, d)
  return x, initial_codebook(x, num_bins)


# ---------------------------------------------------------------- restatement
def initial_codebook(x, num_bins):
  """The rows floor(i * b / m), m = min(num_bins, b, 4096), without those that
  hold a NaN, behind the zero vector; bitwise duplicates removed (the first
  stays, -0.0 is 0.0); at most 4096 rows.  float64 (k, d)."""
  b, d = x.shape
  m = min(int(num_bins), b, MAX_CODEWORDS)
  rows, seen = [], set()
  for row in [np.zeros(d, np.float32)] + [x[(i * b) // m] for i in range(m)]:
    if np.isnan(row).any():
      continue
    row = np.where(row == 0, np.float32(0.0), row).astype(np.float32)
    key = row.tobytes()
    if key not in seen:
      seen.add(key)
      rows.append(row)
  return np.array(rows[:MAX_CODEWORDS], dtype=np.float64)


def distances(x, codebook):
  """(rows, k) float64: the squared distances of the header, started from 0.0
  and accumulated over the components in ascending order, one at a time."""
  xs = x.astype(np.float64)
  dist = np.zeros((x.shape[0], codebook.shape[0]))
  for t in range(x.shape[1]):
    e = xs[:, t, None] - codebook[None, :, t]
    dist = dist + e * e
  return dist


def assign(x, codebook, k, lengths=None, lam=0.0):
  """(indices int32 [b], smallest margin, the squared distance of every row to
  its codeword).  Rows with a NaN get -1 and distance 0."""
  kk = int(np.asarray(k).reshape(-1)[0])
  dist = distances(x, codebook[:kk])
  cost = dist if lam == 0 else dist + lam * lengths[None, :kk]
  ok = ~np.isnan(x).any(1)
  best = np.argmin(np.where(ok[:, None], cost, 0.0), axis=1)
  indices = np.where(ok, best, -1).astype(np.int32)
  chosen = np.where(ok, dist[np.arange(len(best)), best], 0.0)
  return indices, qdata.margin_of(cost[ok]), chosen


def dequantize(indices, codebook):
  picked = codebook[np.maximum(indices, 0)]
  return np.where((indices < 0)[:, None], np.nan, picked).astype(np.float32)


def index_counts(indices, kmax):
  keep = indices[(indices >= 0) & (indices < kmax)]
  return np.bincount(keep, minlength=kmax).astype(np.int64)


def zero_point(codebook, k):
  is_zero = (codebook[:int(k)] == 0.0).all(1)
  return np.int32(is_zero.argmax() if is_zero.any() else -1)


def initial_state(x, codebook):
  """The state vector_lloyd starts from: the lengths and counts of the
  nearest-codeword assignment; kmax is the number of rows of `codebook`."""
  kmax = codebook.shape[0]
  indices, margin, _ = assign(x, codebook, kmax)
  counts = index_counts(indices, kmax)
  with np.errstate(divide='ignore'):
    lengths = -np.log2(counts / np.float64(counts.sum()))
  return {'codebook': codebook.astype(np.float64).copy(), 'lengths': lengths,
          'counts': counts, 'cost': np.zeros(3),
          'k': np.array([kmax], np.int32),
          'zero_index': np.array([zero_point(codebook, kmax)], np.int32),
          'active': np.ones(1, np.int32),
          'iterations': np.zeros(1, np.int32)}, margin


def step(x, state, lam, epsilon, pin_zero):
  """(new state, facts): one Lloyd step of the header.  facts: 'margin' of the
  assignment, 'convergence' = (J_prev - J, epsilon * J_prev) when the test was
  made, 'moved' = rows assigned away from their nearest codeword, 'lost' =
  cells dropped, 'zero_share' = share of the rows in the zero cell."""
  new = {name: value.copy() for name, value in state.items()}
  facts = {'margin': np.inf, 'convergence': None, 'moved': 0, 'lost': 0,
           'zero_share': None}
  if not state['active'][0]:
    return new, facts
  d = x.shape[1]
  k0, z = int(state['k'][0]), int(state['zero_index'][0])
  book, lengths = state['codebook'][:k0], state['lengths'][:k0]
  indices, facts['margin'], dist = assign(x, book, k0, lengths, lam)
  if lam != 0:
    nearest, _, _ = assign(x, book, k0)
    facts['moved'] = int((nearest != indices).sum())
  member = indices >= 0
  n = index_counts(indices, k0)
  total = int(n.sum())
  new['iterations'][0] = state['iterations'][0] + 1
  if total == 0:
    new['cost'][:] = np.nan
    new['active'][0] = 0
    return new, facts
  xs = x.astype(np.float64)
  sums = np.zeros((k0, d))
  for t in range(d):
    sums[:, t] = np.bincount(indices[member], weights=xs[member, t],
                             minlength=k0)
  D = float(dist[member].sum())
  R = float(sum(float(n[i]) * lengths[i] for i in range(k0) if n[i]))
  J = D if lam == 0 else D + lam * R
  pinned = bool(pin_zero) and 0 <= z < k0
  keep = [i for i in range(k0) if n[i] > 0 or (pinned and i == z)]
  for name in ('codebook', 'lengths', 'counts'):
    new[name][...] = 0
  for p, i in enumerate(keep):
    new['codebook'][p] = 0.0 if pinned and i == z else sums[i] / float(n[i])
    new['lengths'][p] = (-np.log2(float(n[i]) / float(total)) if n[i]
                         else np.inf)
    new['counts'][p] = n[i]
  new['k'][0] = len(keep)
  new['zero_index'][0] = -1
  if 0 <= z < k0 and z in keep and (new['codebook'][keep.index(z)] == 0).all():
    new['zero_index'][0] = keep.index(z)
  new['cost'][:] = (J, D, R)
  facts['lost'] = k0 - len(keep)
  if 0 <= z < k0:
    facts['zero_share'] = n[z] / float(x.shape[0])
  done = False
  if state['iterations'][0] > 0:
    J_prev = state['cost'][0]
    facts['convergence'] = (J_prev - J, epsilon * J_prev)
    done = (J_prev - J) <= epsilon * J_prev
  new['active'][0] = 0 if done else 1
  return new, facts


def fit(x, codebook, lam, max_iterations, epsilon, pin_zero):
  """(final state, list of the facts of every step, margin of the initial
  assignment)."""
  state, first_margin = initial_state(x, codebook)
  history = []
  for _ in range(max_iterations):
    state, facts = step(x, state, lam, epsilon, pin_zero)
    history.append(facts)
  return state, history, first_margin


def run_fit(name):
  lam, max_iterations, epsilon, pin_zero = FITS[name][4:]
  x, codebook = fit_inputs(name)
  return fit(x, codebook, lam, max_iterations, epsilon, pin_zero)


# ------------------------------------------------------------ the R-D scene
# the experiment's clusters (experiments/rate_distortion_sparse_coding.py:722):
# 41 coefficients with a scalar quantiser each, the other 23 as one vector
SCAL_CLUSTS = [15, 1, 27, 44, 20, 25, 37, 63, 2, 21, 16, 42, 10, 40, 50, 55,
               34, 62, 35, 51, 58, 47, 9, 52, 11, 14, 46, 49, 13, 26, 5, 60,
               61, 8, 3, 7, 57, 12, 6, 54, 41]
VEC_CLUST = [0, 4, 17, 18, 19, 22, 23, 24, 28, 29, 30, 31, 32, 33, 36, 38, 39,
             43, 45, 48, 53, 56, 59]
PATCH = 8
SCAL_WIDTH = 5.0
# name -> (variant, scal_quant_multiplier, vec_quant_multiplier)
POINTS = {'mod2': (2, 2.0, 3000.0), 'mod3': (3, 2.0, 3000.0)}
RD_ITERATIONS, RD_EPSILON = 6, 1e-3


def scene():
  """Two 32 x 32 single-channel images side by side, their 32 tiled 8 x 8
  patches, a seeded 64 x 64 dictionary with unit rows, and codes made sparse by
  thresholding patches @ dictionary.T.  (With 32 rows a Lagrange
  multiplier has to be large before two cells of the vector quantiser merge:
  the multipliers of POINTS are sized for this scene, not the experiment's.)"""
  rs = np.random.RandomState(50)
  v, u = np.mgrid[0:32, 0:64]
  image = (60 * np.sin(v / 5.0) * np.cos(u / 7.0) + 0.5 * v - 0.3 * u +
           4 * rs.randn(32, 64)).astype(np.float32)
  positions = [(i * PATCH, base + j * PATCH) for base in (0, 32)
               for i in range(4) for j in range(4)]
  patches = np.array([image[r:r + PATCH, c:c + PATCH].reshape(-1)
                      for r, c in positions], dtype=np.float32)
  dictionary = rs.randn(64, 64)
  dictionary /= np.linalg.norm(dictionary, axis=1, keepdims=True)
  dictionary = dictionary.astype(np.float32)
  codes = (patches.astype(np.float64) @ dictionary.astype(np.float64).T)
  threshold = np.full(64, 25.0)
  threshold[VEC_CLUST] = 50.0              # the vector cluster: the sparse tail
  codes[np.abs(codes) < threshold[None, :]] = 0.0
  return {'image': image, 'positions': positions, 'patches': patches,
          'dictionary': dictionary, 'codes': codes.astype(np.float32)}


def uniform_codebooks(x, widths):
  """utils.quantization.uniform_codebooks over the range of every column."""
  lo, hi = x.min(0).astype(np.float64), x.max(0).astype(np.float64)
  w = np.broadcast_to(np.asarray(widths, np.float64), lo.shape)
  m_lo, m_hi = np.rint(lo / w), np.rint(hi / w)
  k = (m_hi - m_lo + 1).astype(np.int32)
  books = np.full((len(k), int(k.max())), np.inf)
  for j in range(len(k)):
    books[j, :k[j]] = (m_lo[j] + np.arange(k[j], dtype=np.float64)) * w[j]
  return books, k


def entropy_bits(counts):
  counts = np.atleast_2d(counts).astype(np.float64)
  n = counts.sum(1, keepdims=True)
  with np.errstate(divide='ignore', invalid='ignore'):
    return float(np.where(counts > 0, -counts * np.log2(counts / n),
                          0.0).sum(1).sum())


def psnr(target, reconstruction):
  """utils.plotting.compute_pSNR in float64."""
  t, r = target.astype(np.float64), reconstruction.astype(np.float64)
  return float(10 * np.log10((t.max() - t.min()) ** 2 / ((t - r) ** 2).mean()))


def mixed_point(s, scal_books, scal_k, scal_lengths, scal_lam, vec_state,
                vec_lam):
  """compute_RD_point_mixed: rate, the dequantised codes, the pSNR of the
  patches and the smallest margin of the assignments."""
  codes = s['codes']
  scal_indices, margin = qdata.assign(codes[:, SCAL_CLUSTS], scal_books,
                                      scal_k, scal_lengths, scal_lam)
  vec_indices, vec_margin, _ = assign(
      codes[:, VEC_CLUST], vec_state['codebook'], vec_state['k'],
      vec_state['lengths'], vec_lam)
  deq = np.zeros(codes.shape, np.float32)
  deq[:, SCAL_CLUSTS] = qdata.dequantize(scal_indices, scal_books)
  deq[:, VEC_CLUST] = dequantize(vec_indices, vec_state['codebook'])
  bits = (entropy_bits(qdata.index_counts(scal_indices, scal_books.shape[1])) +
          entropy_bits(index_counts(vec_indices,
                                    vec_state['codebook'].shape[0])))
  back = deq.astype(np.float64) @ s['dictionary'].astype(np.float64)
  return {'rate': bits / float(s['patches'].size), 'dequantized': deq,
          'psnr_patches': psnr(s['patches'], back),
          'margin': min(margin, vec_margin)}


def rd_point(name, s=None):
  """The training call of Mod2 / Mod3_compute_RD_point on the scene: the
  dictionary of mixed_point plus 'vec' (the fitted vector state), 'scal' (the
  scalar quantiser: 'codebooks', 'k', and for Mod3 the fitted state)."""
  variant, scal_mult, vec_mult = POINTS[name]
  s = scene() if s is None else s
  scal_codes = s['codes'][:, SCAL_CLUSTS]
  margins = []
  if variant == 2:
    books, k = uniform_codebooks(scal_codes, SCAL_WIDTH * scal_mult)
    scal = {'codebooks': books, 'k': k}
    scal_lengths, scal_lam = None, 0.0
  else:
    scal, history, first = qdata.fit(
        scal_codes, *uniform_codebooks(scal_codes, SCAL_WIDTH), scal_mult,
        RD_ITERATIONS, RD_EPSILON, True)
    margins += [first] + [facts['margin'] for facts in history]
    books, k = scal['codebooks'], scal['k']
    scal_lengths, scal_lam = scal['lengths'], scal_mult
  vec_x = s['codes'][:, VEC_CLUST]
  vec, history, first = fit(vec_x, initial_codebook(vec_x, MAX_CODEWORDS),
                            vec_mult, RD_ITERATIONS, RD_EPSILON, True)
  margins += [first] + [facts['margin'] for facts in history]
  point = mixed_point(s, books, k, scal_lengths, scal_lam, vec, vec_mult)
  point['margin'] = min([point['margin']] + margins)
  point.update(vec=vec, scal=scal)
  return point


# ------------------------------------------------------------------ conditions
def conditions(results, points):
  """The facts that keep the fixtures discriminating, over the dict name ->
  (state, history, first_margin) of every fit of FITS and the dict of the R-D
  points."""
  out = {'margin': np.inf, 'convergence_gap': np.inf, 'lost_steps': 0,
         'early': 0, 'late': 0, 'moved': 0, 'zero_share': np.inf,
         'unzeroed': 0}
  for name, (state, history, first_margin) in results.items():
    max_iterations = FITS[name][5]
    out['margin'] = min([out['margin'], first_margin] +
                        [facts['margin'] for facts in history])
    for facts in history:
      out['moved'] += facts['moved']
      out['lost_steps'] += int(facts['lost'] > 0)
      if name in SPARSE and facts['zero_share'] is not None:
        out['zero_share'] = min(out['zero_share'], facts['zero_share'])
      if facts['convergence'] is not None:
        gain, bound = facts['convergence']
        if gain == 0 and bound == 0:
          continue   # J_prev = J = 0 exactly: 0 <= 0
        out['convergence_gap'] = min(out['convergence_gap'],
                                     abs(gain - bound) / (1e-6 * abs(bound)))
    out['early'] += int(state['active'][0] == 0 and
                        state['iterations'][0] < max_iterations)
    out['late'] += int(state['active'][0] != 0)
    out['unzeroed'] += int(state['zero_index'][0] < 0)
  for point in points.values():
    out['margin'] = min(out['margin'], point['margin'])
  return out


def check_conditions(facts):
  assert facts['margin'] > MARGIN, facts
  assert facts['convergence_gap'] > 1.0, facts
  assert facts['lost_steps'] >= 1, facts
  assert facts['early'] >= 1 and facts['late'] >= 1, facts
  assert facts['moved'] >= 1, facts
  assert facts['zero_share'] > 0.5, facts
  assert facts['unzeroed'] >= 1, facts   # an unpinned zero cell moved away
