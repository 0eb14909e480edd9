"""Cases, dispatch mirror and float64 references behind
tests/test_subspace_routes_gpu.py and tests/test_subspace_gates_host.py.

vtc_subspace_ista_fista (csrc/subspace.hip) picks a kernel family, an operand
split, a one-pass or split-K residual product and one of three proximal steps
from (b, n, groups, m, precision, early stopping, CU count).  subspace_route
restates that choice; every case below names the tuple it must give.  Nothing
here needs a GPU."""
import collections
import functools

import numpy as np
import torch

import helpers
import sc_oracle

ceil_div = lambda a, b: -(-a // b)

T = 12                  # iterations of every plain case
SAMPLE = 256            # rows that meet the oracle when b > SAMPLE_ABOVE
SAMPLE_ABOVE = 512
EDGE_ROWS = 8           # the batch's last rows are always in the sample
WARM_FROM, WARM_ITERS = 5, 7
STOP_ITERS = 200
ACTIVE_BAND = (0.1, 0.9)

GATE_F32 = (helpers.REL_TOL_SHORT, helpers.NEAR_THRESHOLD)
GATE_BF16 = (2e-5, 1e-5)     # tests/test_subspace_gpu.py


# ------------------------------------------------------------ dispatch mirror
def x3_want_slices(M, N, K):
  """gemm_x3_want_slices (csrc/gemm_x3.h), as in tests/test_large_batch_gpu.py:
  K slices of a split-precision product with few 128 x 128 output tiles."""
  want = min(ceil_div(512, ceil_div(M, 128) * ceil_div(N, 128)),
             ceil_div(K, 256), 16)
  want = max(want, 1)
  chunk = max(ceil_div(ceil_div(K, want), 32) * 32, 32)
  return ceil_div(K, chunk)


def gemm_prefers_small(m, n, cus):
  """gemm_prefers_small (csrc/gemm_f32.h): 128 x 128 tiles."""
  return ceil_div(m, 128) * ceil_div(n, 128) <= 8 or m * n / 16384. <= cus


def subspace_route(b, n, groups, m, precision, eps, cus):
  """(family, split, residual, prox) of vtc_subspace_ista_fista for 16-byte
  aligned operands.  The streamed kernel carries its products and its proximal
  step itself: residual and prox are None there."""
  slots = groups * m
  if (precision != 'f32' and eps is None and n == 256 and slots % 256 == 0 and
      slots <= 16384 and m in (1, 2, 4, 8)):       # stream_shape_supported
    return ('stream', 'f16' if precision == 'f16x3' else 'bf16', None, None)
  pow2 = m in (1, 2, 4, 8, 16, 32)
  if precision == 'f32':
    split = 'f32'
  else:
    assert n % 4 == 0 and slots % 4 == 0, 'the split modes refuse this shape'
    split = 'f16' if precision == 'f16x3' and pow2 else 'bf16'
  residual = 'split-k' if (split != 'f32' and
                           x3_want_slices(b, n, slots) > 1) else 'single'
  if slots % 4 == 0 and pow2 and (
      split != 'f32' or not gemm_prefers_small(b, slots, cus)):
    prox = 'epilogue'
  elif m in (1, 2, 4, 8, 16, 32, 64) and b * slots % 4 == 0:
    prox = 'pow2-kernel'
  else:
    prox = 'group-kernel'
  return ('tiled', split, residual, prox)


def gate(route):
  """(relative l2 error, largest tolerated support flip) of a route."""
  return GATE_BF16 if route[1] == 'bf16' else GATE_F32


# ---------------------------------------------------------------------- cases
# b: a number, or ('cut-over', slots, extra): the first batch at which
# b * slots passes 16384 * CUs (gemm_prefers_small gives way), plus extra.
# stop_eps: early-stopping epsilon of the options test, None where the case
# has no options.
Case = collections.namedtuple(
    'Case', 'name precision m layout groups b n lam route stop_eps')

CUT = lambda slots, extra: ('cut-over', slots, extra)
E32 = ('tiled', 'f32', 'single', 'epilogue')
P32 = ('tiled', 'f32', 'single', 'pow2-kernel')
G32 = ('tiled', 'f32', 'single', 'group-kernel')


def _cases():
  out = []
  add = lambda *a: out.append(Case(*a))
  # 1: exact-f32 whole-tile epilogue, 1056 slots = 33 column tiles of 32
  for m, lam, eps in ((1, 0.03, None), (2, 0.045, None), (4, 0.06, None),
                      (8, 0.1, 3.95e-3), (16, 0.12, None), (32, 0.15, None)):
    add('1 f32 epilogue m=%d' % m, 'f32', m, 'contiguous', 1056 // m,
        CUT(1056, 105), 24, lam, E32, eps)
  # 2: group_prox_pow2_kernel<16 / 32 / 64> in f32
  for m, lam in ((16, 0.12), (32, 0.15), (64, 0.3)):
    for b in (40, 300):
      add('2 f32 pow2 kernel m=%d b=%d' % (m, b), 'f32', m, 'contiguous', 12,
          b, 24, lam, P32, None)
  # 3: more than 8192 * 256 quads: the rounds loop of group_prox_pow2_kernel
  add('3 f32 pow2 kernel multi-round m=64', 'f32', 64, 'contiguous', 66, 2000,
      16, 0.6, P32, 2.57e-3)
  add('3 bf16x3 pow2 kernel multi-round m=64', 'bf16x3', 64, 'contiguous', 66,
      2000, 16, 0.6, ('tiled', 'bf16', 'split-k', 'pow2-kernel'), None)
  # 4, 5: more than 4096 * 256 (patch, group) pairs: the stride loop of
  # group_prox_kernel, behind the 32 x 32 and the 128 x 128 f32 kernel
  add('4 f32 group kernel stride loop m=3', 'f32', 3, 'contiguous', 40, 26500,
      16, 0.05, G32, 4.8e-3)
  add('5 f32 group kernel large tiles m=3', 'f32', 3, 'contiguous', 40,
      CUT(120, 37), 16, 0.05, G32, None)
  # 6: powers of two whose b * slots is no multiple of 4
  for m, lam in ((1, 0.03), (2, 0.08)):
    add('6 f32 group kernel fallback m=%d' % m, 'f32', m, 'contiguous', 7, 3,
        24, lam, G32, None)
  # 7: split epilogue over 2 1/3 row tiles
  for prec in ('bf16x3', 'f16x3'):
    for m, lam in ((1, 0.03), (2, 0.045), (16, 0.25), (32, 0.4)):
      add('7 %s epilogue m=%d' % (prec, m), prec, m, 'contiguous',
          20 if m <= 16 else 5, 300, 64, lam,
          # 320 slots: the residual product splits its K axis in two
          ('tiled', prec[:-2], 'split-k' if m == 16 else 'single',
           'epilogue'), 3.7e-3 if m == 16 else None)
  # 8: split-K residual ahead of the epilogue
  for prec in ('bf16x3', 'f16x3'):
    for m, lam in ((1, 0.03), (32, 0.2)):
      add('8 %s split-K m=%d' % (prec, m), prec, m, 'contiguous', 544 // m,
          70, 64, lam, ('tiled', prec[:-2], 'split-k', 'epilogue'), None)
  # 9: ragged, overlapping groups, padded to m = 4
  add('9 f32 ragged overlapping', 'f32', 4, 'ragged-3-1-4', 264,
      CUT(1056, 105), 24, 0.05, E32, None)
  add('9 f16x3 ragged overlapping', 'f16x3', 4, 'ragged-3-1-4', 264, 300, 24,
      0.05, ('tiled', 'f16', 'split-k', 'epilogue'), None)
  # 10: the streamed kernel through the plugin
  add('10 stream m=1', 'f16x3', 1, 'contiguous', 768, 45, 256, 0.02,
      ('stream', 'f16', None, None), None)
  add('10 stream ragged 8-5-3', 'f16x3', 8, 'ragged-8-5-3', 96, 45, 256, 0.05,
      ('stream', 'f16', None, None), None)
  return out


CASES = _cases()
BY_NAME = dict((c.name, c) for c in CASES)
OPTION_CASES = [c for c in CASES if c.stop_eps is not None]


def batch_size(case, cus):
  if isinstance(case.b, tuple):
    _, slots, extra = case.b
    return ceil_div(16384 * cus, slots) + extra
  return case.b


def group_lists(case):
  """(groups, number of atoms)."""
  m, count = case.m, case.groups
  if case.layout == 'contiguous':
    return [list(range(g * m, g * m + m)) for g in range(count)], count * m
  sizes = {'ragged-3-1-4': (3, 1, 4), 'ragged-8-5-3': (8, 5, 3)}[case.layout]
  overlap = case.layout == 'ragged-3-1-4'
  groups, atoms = [], 0
  for g in range(count):
    size = sizes[g % len(sizes)]
    members = []
    if overlap and g % 3 == 2:      # shares its neighbour's last atom
      members.append(groups[-1][-1])
    while len(members) < size:
      members.append(atoms)
      atoms += 1
    groups.append(members)
  assert max(len(g) for g in groups) == m
  return groups, atoms


def sample_rows(seed, b):
  """A seeded sorted sample of SAMPLE rows (tests/test_large_batch_gpu.py
  _sample) that always holds the batch's last EDGE_ROWS rows: the ragged row
  tile is where a tiled kernel goes wrong first."""
  if b <= SAMPLE_ABOVE:
    return np.arange(b)
  rows = np.random.RandomState(seed).choice(b - EDGE_ROWS,
                                            size=SAMPLE - EDGE_ROWS,
                                            replace=False)
  rows = np.concatenate([rows, np.arange(b - EDGE_ROWS, b)])
  rows.sort()
  return rows


Problem = collections.namedtuple(
    'Problem', 'case b groups atoms slots X D eta rows valid index')


@functools.lru_cache(maxsize=None)
def problem(name, cus):
  case = BY_NAME[name]
  seed = 7000 + 10 * CASES.index(case)
  b = batch_size(case, cus)
  groups, atoms = group_lists(case)
  X = helpers.gaussian_patches(seed, b, case.n)
  D = helpers.unit_rows(seed + 1, atoms, case.n)
  dg = sc_oracle.grouped_dictionary(torch.from_numpy(D).double(), groups)
  eta = float(1. / sc_oracle.largest_eigenvalue(torch.mm(dg.t(), dg)))
  index, valid, _, m = sc_oracle.group_layout(groups, atoms)
  assert m == case.m
  return Problem(case, b, groups, atoms, case.groups * case.m, X, D, eta,
                 sample_rows(seed + 2, b), valid.numpy(), index.numpy())


def oracle(p, dtype, num_iters, variant='fista', rows=None, **kw):
  X = p.X if rows is None else p.X[rows]
  return sc_oracle.subspace_ista_fista(
      torch.from_numpy(X).to(dtype), torch.from_numpy(p.D).to(dtype), p.groups,
      p.case.lam, num_iters, variant=variant, stepsize=p.eta, **kw)


def active_fraction(p, codes):
  """Fraction of (row, group) pairs with a non-zero member."""
  nz = np.asarray(codes) != 0
  if p.case.layout == 'contiguous':
    return float(nz.reshape(nz.shape[0], p.case.groups, p.case.m).any(
        axis=2).mean())
  return float(np.mean([nz[:, g].any(axis=1).mean() for g in p.groups]))


def assert_input_conditions(p, ref64, ref32, what):
  """The case is not degenerate (a share of the groups is active, a share is
  not) and float32 arithmetic reaches half the gate with no support flip above
  NEAR_THRESHOLD: the gate leaves room for the kernels' rounding and none for
  a wrong one."""
  lo, hi = ACTIVE_BAND
  frac = active_fraction(p, ref64)
  assert lo <= frac <= hi, '%s: %.3f of the groups active' % (what, frac)
  err, _ = helpers.assert_codes_match(
      ref32, ref64, gate(p.case.route)[0] / 2, what + ': float32 oracle',
      max_flip_mag=helpers.NEAR_THRESHOLD)
  return frac, err


@functools.lru_cache(maxsize=None)
def reference(name, cus, variant='fista'):
  """(float64 codes, float32 codes) of the sampled rows after T iterations."""
  p = problem(name, cus)
  return (oracle(p, torch.float64, T, variant, p.rows).numpy(),
          oracle(p, torch.float32, T, variant, p.rows).numpy())


def warm_reference(name, cus):
  """(initial codes of the whole batch as float32, float64 and float32 codes
  of the sampled rows WARM_ITERS iterations later)."""
  p = problem(name, cus)
  init = oracle(p, torch.float64, WARM_FROM).float()
  refs = [oracle(p, dtype, WARM_ITERS, rows=p.rows,
                 initial_codes=init[p.rows].to(dtype)).numpy()
          for dtype in (torch.float64, torch.float32)]
  return init.numpy(), refs[0], refs[1]


def stop_count(p, dtype, eps):
  codes, trace = oracle(p, dtype, STOP_ITERS, 'ista',
                        early_stopping_epsilon=eps,
                        trace_at=set(range(1, STOP_ITERS + 1)))
  return codes.numpy(), len(trace)


def stop_reference(name, cus):
  """Early stopping is a mean over the whole batch: the oracle runs on all of
  it.  Returns (float64 codes, float32 codes, iteration count); the count is
  the same for 0.99 eps and 1.01 eps, so it does not hinge on a rounding."""
  p = problem(name, cus)
  eps = p.case.stop_eps
  ref64, count = stop_count(p, torch.float64, eps)
  ref32, count32 = stop_count(p, torch.float32, eps)
  assert 1 < count < STOP_ITERS, count
  assert count32 == count
  for factor in (0.99, 1.01):
    assert stop_count(p, torch.float64, factor * eps)[1] == count, factor
  return ref64, ref32, count


# ------------------------------------------ float64 iteration in grouped form
def grouped_iterates(p, rows, num_iters, variant='fista'):
  """The padded (rows, slots) codes after every iteration, float64: what the
  kernels hold before scatter_add_kernel sums an atom's slots.  Returns
  (codes per iteration, evaluation points per iteration, Dg)."""
  dg = p.D.astype(np.float64)[p.index] * p.valid[:, None]
  X = p.X[rows].astype(np.float64)
  betas = sc_oracle.fista_betas(num_iters)
  c_prev = np.zeros((len(rows), p.slots))
  y = c_prev.copy()
  codes, points = [], []
  for k in range(num_iters):
    points.append(y)
    c = group_step(p, X, dg, y)
    y = c + betas[k] * (c - c_prev) if variant == 'fista' else c
    c_prev = c
    codes.append(c)
  return codes, points, dg


def group_step(p, X, dg, y, norms_of=None):
  """One gradient and proximal step from the evaluation point y; norms_of
  (pre-shrink values -> per-slot group norm) lets a test swap the norm."""
  pre = y - p.eta * ((y @ dg - X) @ dg.T)
  if norms_of is None:
    norms_of = lambda v: group_norms(p, v)
  norms = norms_of(pre)
  norms = np.where(norms == 0, 1.0, norms)
  return pre * np.maximum(1 - p.case.lam * p.eta / norms, 0.)


def group_norms(p, pre, members=None):
  """Per-slot l2 norm of the slot's group, over its first `members` slots."""
  m = p.case.m
  g = pre.reshape(pre.shape[0], -1, m)
  nrm = np.sqrt((g[:, :, :members] ** 2).sum(axis=2, keepdims=True))
  return np.broadcast_to(nrm, g.shape).reshape(pre.shape)


def scatter(p, grouped, masked=True):
  """scatter_add_kernel: an atom's code is the sum over its valid slots;
  masked=False adds the padded slots (index 0) as well."""
  out = np.zeros((grouped.shape[0], p.atoms), grouped.dtype)
  keep = np.nonzero(p.valid)[0] if masked else np.arange(p.slots)
  np.add.at(out, (slice(None), p.index[keep]), grouped[:, keep])
  return out
