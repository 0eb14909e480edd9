"""Seeded inputs of the quantisation tests and the float64 numpy restatement
of the contract of include/vtc_quant.h: assign, one Lloyd step, a fit.  The
reference has no utils.quantization to compare against, so this restatement
is the truth of tests/golden/quantization.npz (tools/make_quantization_golden.py)
and of the GPU tests.  It is test infrastructure, like tests/ssim_oracle.py.

A quantiser state is a dict of numpy arrays: codebooks, lengths float64
(s, kmax), counts int64 (s, kmax), cost float64 (s, 3), k, zero_index, active,
iterations int32 [s].  Slots past k are never read; a step writes 0.0, 0.0, 0
there.
"""
import numpy as np

ROWS = 512            # VTC_QUANT_ROWS
MAX_CODEWORDS = 1024  # VTC_QUANT_MAX_CODEWORDS
MARGIN = 1e-8         # second-best cost - best > MARGIN * (1 + best)

STATE_FLOAT = ('codebooks', 'lengths', 'cost')
STATE_INT = ('counts', 'k', 'zero_index', 'active', 'iterations')


# --------------------------------------------------------------------- inputs
def codes(seed, b, s, zeros=0.7):
  """Laplace codes, a share `zeros` of them exactly 0.0, the scale and the
  sparsity varying with the column; float32."""
  rs = np.random.RandomState(seed)
  x = rs.laplace(size=(b, s)) * (0.5 + 0.5 * (np.arange(s) % 5))
  share = np.clip(zeros + 0.25 * ((np.arange(s) % 3) - 1), 0.0, 0.97)
  x[rs.rand(b, s) < share] = 0.0
  return x.astype(np.float32)


def grid_codebooks(s, k, width):
  """Every column: the k codewords (i - k // 2) * width.  (codebooks, k)."""
  values = (np.arange(k, dtype=np.float64) - k // 2) * width
  return np.tile(values, (s, 1)), np.full(s, k, np.int32)


# name -> (seed, b, s, k, width, lambda, max_iterations, epsilon, pin_zero)
FITS = {
    'one':        (11, 1, 1, 1, 1.0, 0.0, 3, 1e-3, True),
    'two':        (12, 65, 3, 2, 1.0, 0.0, 4, 1e-3, True),
    'grid33':     (13, ROWS + 3, 67, 33, 0.375, 0.0, 6, 1e-3, True),
    'grid33_ec':  (14, ROWS + 3, 67, 33, 0.375, 0.05, 6, 1e-3, True),
    'unpinned':   (15, 65, 67, 33, 0.375, 0.02, 5, 1e-3, False),
    'full':       (16, ROWS + 3, 3, 1024, 1.0 / 64, 0.0, 3, 1e-3, True),
}


def fit_inputs(name):
  seed, b, s, k, width = FITS[name][:5]
  return (codes(seed, b, s),) + grid_codebooks(s, k, width)


# ---------------------------------------------------------------- restatement
def zero_points(codebooks, k):
  is_zero = (codebooks == 0.0) & (np.arange(codebooks.shape[1])[None, :]
                                  < k[:, None])
  return np.where(is_zero.any(1), is_zero.argmax(1), -1).astype(np.int32)


def column_costs(x, codebook, lengths, lam):
  """(rows, k) float64: d * d + lam * length, the length term left out when
  lam == 0."""
  d = x.astype(np.float64)[:, None] - codebook[None, :]
  cost = d * d
  if lam != 0:
    cost = cost + lam * lengths[None, :]
  return cost


def margin_of(cost):
  """min over rows of (second best - best) / (1 + best); inf with one cell."""
  if cost.shape[1] < 2 or not cost.shape[0]:
    return np.inf
  two = np.partition(cost, 1, axis=1)[:, :2]
  with np.errstate(invalid='ignore'):
    gap = (two[:, 1] - two[:, 0]) / (1 + two[:, 0])
  return float(np.nanmin(np.where(np.isinf(two[:, 1]), np.inf, gap)))


def assign(x, codebooks, k, lengths=None, lam=0.0, active=None):
  """(indices int32 (b, s), smallest margin).  NaN codes get -1; columns with
  active == 0 get -2 (not assigned)."""
  b, s = x.shape
  indices = np.full((b, s), -2, np.int32)
  margin = np.inf
  for j in range(s):
    if active is not None and not active[j]:
      continue
    kk = int(k[j])
    cost = column_costs(x[:, j], codebooks[j, :kk],
                        None if lengths is None else lengths[j, :kk], lam)
    ok = ~np.isnan(x[:, j])
    indices[:, j] = np.where(ok, np.argmin(np.where(ok[:, None], cost, 0.0),
                                           axis=1), -1)
    margin = min(margin, margin_of(cost[ok]))
  return indices, margin


def dequantize(indices, codebooks):
  picked = np.take_along_axis(codebooks.T, np.maximum(indices, 0), axis=0)
  return np.where(indices < 0, np.nan, picked).astype(np.float32)


def index_counts(indices, kmax):
  s = indices.shape[1]
  counts = np.zeros((s, kmax), np.int64)
  for j in range(s):
    col = indices[:, j]
    col = col[(col >= 0) & (col < kmax)]
    counts[j] = np.bincount(col, minlength=kmax)
  return counts


def initial_state(x, codebooks, k):
  """The state scalar_lloyd starts from: the lengths and counts of the
  nearest-codeword assignment."""
  s, kmax = codebooks.shape
  indices, margin = assign(x, codebooks, k)
  counts = index_counts(indices, kmax)
  with np.errstate(divide='ignore'):
    lengths = -np.log2(counts / counts.sum(1, keepdims=True).astype(np.float64))
  padded = np.where(np.arange(kmax)[None, :] < k[:, None], codebooks, np.inf)
  return {'codebooks': padded, 'lengths': lengths, 'counts': counts,
          'cost': np.zeros((s, 3)), 'k': k.astype(np.int32),
          'zero_index': zero_points(codebooks, k),
          'active': np.ones(s, np.int32),
          'iterations': np.zeros(s, np.int32)}, margin


def step(x, state, lam, epsilon, pin_zero):
  """(new state, facts): one Lloyd step of the header.  facts: 'margin' of the
  assignment, 'convergence' = list of (J_prev - J, epsilon * J_prev) of the
  columns that made the test, 'moved' = elements assigned away from their
  nearest codeword."""
  s, kmax = state['codebooks'].shape
  new = {name: value.copy() for name, value in state.items()}
  indices, margin = assign(x, state['codebooks'], state['k'],
                           state['lengths'], lam, state['active'])
  facts = {'margin': margin, 'convergence': [], 'moved': 0}
  if lam != 0:
    nearest, _ = assign(x, state['codebooks'], state['k'], None, 0.0,
                        state['active'])
    facts['moved'] = int((nearest != indices).sum())
  for j in range(s):
    if not state['active'][j]:
      continue
    k0, z = int(state['k'][j]), int(state['zero_index'][j])
    xs = x[:, j].astype(np.float64)
    member = indices[:, j]
    n = np.array([(member == i).sum() for i in range(k0)], np.int64)
    total = int(n.sum())
    new['iterations'][j] = state['iterations'][j] + 1
    if total == 0:
      new['cost'][j] = np.nan
      new['active'][j] = 0
      continue
    centre = state['codebooks'][j, :k0]
    sums = np.array([xs[member == i].sum() for i in range(k0)])
    D = sum(((xs[member == i] - centre[i]) ** 2).sum() for i in range(k0))
    R = sum(float(n[i]) * state['lengths'][j, i] for i in range(k0) if n[i])
    J = D if lam == 0 else D + lam * R
    pinned = bool(pin_zero) and 0 <= z < k0
    keep = [i for i in range(k0) if n[i] > 0 or (pinned and i == z)]
    for name in ('codebooks', 'lengths', 'counts'):
      new[name][j] = 0
    for p, i in enumerate(keep):
      new['codebooks'][j, p] = (0.0 if pinned and i == z
                                else sums[i] / float(n[i]))
      new['lengths'][j, p] = (-np.log2(float(n[i]) / float(total)) if n[i]
                              else np.inf)
      new['counts'][j, p] = n[i]
    new['k'][j] = len(keep)
    new['zero_index'][j] = -1
    if 0 <= z < k0 and z in keep and new['codebooks'][j, keep.index(z)] == 0:
      new['zero_index'][j] = keep.index(z)
    new['cost'][j] = (J, D, R)
    done = False
    if state['iterations'][j] > 0:
      J_prev = state['cost'][j, 0]
      facts['convergence'].append((J_prev - J, epsilon * J_prev))
      done = (J_prev - J) <= epsilon * J_prev
    new['active'][j] = 0 if done else 1
  return new, facts


def fit(x, codebooks, k, lam, max_iterations, epsilon, pin_zero):
  """(final state, list of the facts of every step, margin of the initial
  assignment)."""
  state, first_margin = initial_state(x, codebooks, k)
  history = []
  for _ in range(max_iterations):
    state, facts = step(x, state, lam, epsilon, pin_zero)
    history.append(facts)
  return state, history, first_margin


def run_fit(name):
  lam, max_iterations, epsilon, pin_zero = FITS[name][5:]
  x, codebooks, k = fit_inputs(name)
  return fit(x, codebooks, k, lam, max_iterations, epsilon, pin_zero)


def conditions(results):
  """The facts that keep the Lloyd fixtures discriminating, over the dict
  name -> (state, history, first_margin) of every fit of FITS."""
  out = {'margin': np.inf, 'convergence_gap': np.inf, 'lost': 0, 'early': 0,
         'late': 0, 'moved': 0}
  for name, (state, history, first_margin) in results.items():
    x, codebooks, k = fit_inputs(name)
    epsilon, max_iterations = FITS[name][7], FITS[name][6]
    out['margin'] = min([out['margin'], first_margin] +
                        [facts['margin'] for facts in history])
    for facts in history:
      out['moved'] += facts['moved']
      for gain, bound in facts['convergence']:
        if gain == 0 and bound == 0:
          continue   # J_prev = J = 0 exactly (all codes on codewords): 0 <= 0
        # |gain - epsilon J_prev| relative to 1e-6 * epsilon * J_prev
        out['convergence_gap'] = min(out['convergence_gap'],
                                     abs(gain - bound) / (1e-6 * bound))
    out['lost'] += int((state['k'] < k).sum())
    out['early'] += int(((state['active'] == 0) &
                         (state['iterations'] < max_iterations)).sum())
    out['late'] += int((state['active'] != 0).sum())
  return out


def check_conditions(facts):
  assert facts['margin'] > MARGIN, facts
  assert facts['convergence_gap'] > 1.0, facts
  assert facts['lost'] >= 1 and facts['early'] >= 1 and facts['late'] >= 1
  assert facts['moved'] >= 1, facts


# ------------------------------------------------------- uniform codebook cases
# (lo, hi, binwidth) per column: ties of rint, zero inside / outside the range
UNIFORM_LO = np.array([-12.3, 0.0, 2.5, -7.5, -0.2, 4.9, -30.0, np.nan])
UNIFORM_HI = np.array([9.9, 0.0, 7.5, -2.5, 0.2, 25.1, -11.0, np.nan])
UNIFORM_W = np.array([5.0, 5.0, 5.0, 5.0, 0.5, 5.0, 2.0, 1.0])
