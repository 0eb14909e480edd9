"""Cases, dispatch mirror and float64 references behind
tests/test_fc_routes_gpu.py and tests/test_fc_gates_host.py.

vtc_fc_ista_fista (csrc/fc_inference.hip) picks one of five kernel families --
fc_small, fc_chip16, the fused persistent kernel, its streamed-state form, the
tiled loop of run_generic -- from (b, n, s, precision, early stopping, iteration
count, CU count).  fc_route restates that choice for 16-byte aligned operands;
every case below names the tuple it must give.  Nothing here needs a GPU."""
import collections
import functools

import numpy as np
import torch

import helpers
import sc_oracle
from subspace_routes_data import (ceil_div, gemm_prefers_small, sample_rows,
                                  x3_want_slices)

T = 12                  # iterations of every plain case
WARM_FROM, WARM_ITERS = 5, 7
STOP_ITERS = 200
HARD_ITERS_BF16X2 = 3   # hard thresholds on the bf16 hi/lo split
HARD_ITERS_BF16 = 1     # and in the single-part bf16 mode, see reference()
ACTIVE_BAND = (0.1, 0.9)
LEFT_OUT_CAP = 0.15     # rows of a hard-threshold case next to the cutoff
MAX_ITERS_ON_CHIP = 16384   # kBetaTable (csrc/fc_fused.hip): fused_max_iters()

GATE_F32 = (helpers.REL_TOL_SHORT, helpers.NEAR_THRESHOLD)
GATE_BF16X2 = (1e-5, 5e-6)   # SPLIT['bf16x3'] of tests/test_fc_fused_gpu.py
GATE_BF16_CAP = 5e-3         # a tenth of REL_TOL_BF16 of test_fc_fused_gpu.py
# half-width of the band around lam * eta in which a pre-threshold value may
# fall on either side of a hard threshold: a tenth of NEAR_THRESHOLD for f32
# and the f16 split, a fifth of the flip gate for the bf16 splits
NEAR_CUTOFF = {'f32': 2e-7, 'f16': 2e-7, 'bf16x2': 1e-6, 'bf16': 1e-6}

THRESHOLDS = {'soft': (False, False), 'soft_nonneg': (True, False),
              'hard': (False, True), 'hard_nonneg': (True, True)}


# ------------------------------------------------------------ dispatch mirror
def fc_route(b, n, s, precision, eps, num_iters, cus):
  """The kernel family of fc_ista_fista_impl and, on the tiled loop, the
  branches of run_generic, for 16-byte aligned operands.  eps is None without
  early stopping (the C call takes a negative epsilon for that; 0.0 is early
  stopping that never fires)."""
  on_chip = eps is None and num_iters <= MAX_ITERS_ON_CHIP
  # fused_shape_supported: n = 256 and 2, 4 or 8 phases of 128 atoms
  fused_ok = on_chip and precision != 'f32' and n == 256 and s in (
      256, 512, 1024)
  if precision == 'bf16' and not fused_ok:
    return ('refused', 'bf16 exists only as the fused kernel')
  if precision == 'f32' and on_chip:
    if n == 64 and s in (64, 128, 192):              # small_shape_supported
      return ('small', 'f32')
    if (n == 144 and s in (288, 576)) or (n == 64 and s in (256, 512)):
      return ('chip16', 'f32')                       # chip16_shape_supported
  if fused_ok:
    split = {'bf16': 'bf16', 'bf16x3': 'bf16x2', 'f16x3': 'f16'}[precision]
    # default_tile16: f16x3 and bf16 on 16x16x32, bf16x3 on 32x32x16
    return ('fused', split, 32 if precision == 'bf16x3' else 16)
  if (precision != 'f32' and on_chip and n == 256 and s % 256 == 0 and
      s <= 16384):                                   # stream_shape_supported
    return ('stream', 'f16' if precision == 'f16x3' else 'bf16x2')
  if precision == 'f32':
    wide = s % 4 == 0 and not gemm_prefers_small(b, s, cus)
    return ('tiled', 'f32', 'single', 'wide' if wide else 'element')
  if n % 4 or s % 4:
    return ('refused', 'the split tiles need n and s to be multiples of 4')
  return ('tiled', 'f16' if precision == 'f16x3' else 'bf16x2',
          'split-k' if x3_want_slices(b, n, s) > 1 else 'single', 'wide')


def gate(route):
  """(relative l2 error, largest tolerated support flip) of a route.  The
  single-part bf16 mode has a gate per case and option: reference()."""
  assert route[1] != 'bf16'
  return GATE_BF16X2 if route[1] == 'bf16x2' else GATE_F32


# ---------------------------------------------------------------------- cases
# b: a number, or ('cut-over', s, extra): the first batch at which b * s passes
# 16384 * CUs (gemm_prefers_small gives way), plus extra.
# auto: what ista_fista._resolve_precision('auto', ...) gives for the shape
# without early stopping; 'by-size': f16x3 from b * s * n = 2.4e8, f32 below.
# eps: the early-stopping epsilon of every run of the case but 'stop': None, or
# 0.0, which never fires and keeps a fused shape on the tiles.
# stop_eps: early-stopping epsilon of the 'stop' option.
# options: see option_spec.
Case = collections.namedtuple(
    'Case', 'name precision b n s lam route auto eps stop_eps options')

CUT = lambda s, extra: ('cut-over', s, extra)
VARIANTS = ('fista', 'ista')
OTHER_THRESHOLDS = ('soft_nonneg', 'hard', 'hard_nonneg')
SOFT_OPTIONS = ['ista', 'warm', 'fista soft_nonneg', 'ista soft_nonneg']
HARD_OPTIONS = ['%s %s' % (v, t) for t in ('hard', 'hard_nonneg')
                for v in VARIANTS]
TILE_OPTIONS = ['tile fista ' + t for t in OTHER_THRESHOLDS]


def _options(hard=False, stop=False):
  return tuple(SOFT_OPTIONS + (HARD_OPTIONS if hard else []) +
               (['stop'] if stop else []) + ['dev-eta'])


def _cases():
  out = []

  def add(name, precision, b, n, s, lam, route, auto, stop_eps=None,
          options=(), eps=None):
    out.append(Case(name, precision, b, n, s, lam, route, auto, eps, stop_eps,
                    tuple(options)))
  # 1: everything on the CU, exact f32, one and a bit 32-patch groups
  for s in (64, 128, 192):
    add('1 small s=%d' % s, 'f32', 33, 64, s, 0.05, ('small', 'f32'), 'f32',
        options=('warm soft_nonneg', 'dev-eta') if s == 192 else ())
  for n, s in ((144, 288), (144, 576), (64, 256), (64, 512)):
    add('1 chip16 n=%d s=%d' % (n, s), 'f32', 17, n, s, 0.05,
        ('chip16', 'f32'), 'f32',
        options=('warm soft_nonneg', 'dev-eta') if (n, s) == (144, 576) else ())
  # 2: the fused kernel, NPH = 2, 4, 8: two full 32-patch workgroups and one of
  # 5 rows.  Hard thresholds: the f16 split at every s, the bf16 modes at
  # s = 256 and HARD_ITERS_BF16X2 / HARD_ITERS_BF16 iterations (with 1024 atoms
  # more rows than LEFT_OUT_CAP sit next to the cutoff); at s = 256 the three
  # other thresholds also run on the tile that is not the default
  for s in (256, 512, 1024):
    for prec, split, tile in (('f16x3', 'f16', 16), ('bf16x3', 'bf16x2', 32),
                              ('bf16', 'bf16', 16)):
      hard = prec == 'f16x3' or s == 256
      add('2 fused %s s=%d' % (prec, s), prec, 69, 256, s, 0.05,
          ('fused', split, tile), 'f16x3',
          options=_options(hard=hard) + (
              tuple(o for o in TILE_OPTIONS if hard or 'hard' not in o)
              if s == 256 else ()))
  # 3: the streamed kernel: six phases (the fused kernel refuses them), its
  # first shape past the fused ones, its largest
  for prec, split in (('f16x3', 'f16'), ('bf16x3', 'bf16x2')):
    add('3 stream %s s=768' % prec, prec, 45, 256, 768, 0.05,
        ('stream', split), 'f32', options=_options(hard=prec == 'f16x3'))
    add('3 stream %s s=1280' % prec, prec, 45, 256, 1280, 0.05,
        ('stream', split), 'f16x3')
    add('3 stream %s s=16384' % prec, prec, 8, 256, 16384, 0.03,
        ('stream', split), 'f16x3', options=('ista', 'warm'))
  # 4: the exact-f32 tiles.  s % 4 != 0: the element-wise epilogue, nothing a
  # multiple of 32
  add('4 f32 element s=201', 'f32', 130, 100, 201, 0.05,
      ('tiled', 'f32', 'single', 'element'), 'f32', 1.14e-3,
      _options(hard=True, stop=True))
  # the 16-byte epilogue past the cut-over of gemm_prefers_small, a ragged last
  # row tile; the element-wise one behind the 32 x 32-tile product below it
  add('4 f32 wide past the cut-over', 'f32', CUT(200, 37), 100, 200, 0.05,
      ('tiled', 'f32', 'single', 'wide'), 'by-size', 3.63e-3,
      _options(hard=True, stop=True))
  add('4 f32 element below the cut-over', 'f32', CUT(200, -128), 100, 200,
      0.05, ('tiled', 'f32', 'single', 'element'), 'by-size')
  add('4 f32 at a fused shape', 'f32', 45, 256, 1024, 0.05,
      ('tiled', 'f32', 'single', 'element'), 'f16x3')
  # 5: the split tiles
  for prec, split, eps in (('bf16x3', 'bf16x2', (3.60e-3, 2.82e-3, 3.68e-3)),
                           ('f16x3', 'f16', (3.28e-3, 2.75e-3, 3.69e-3))):
    add('5 %s single pass' % prec, prec, 300, 64, 64, 0.05,
        ('tiled', split, 'single', 'wide'), 'f32', eps[0],
        _options(hard=True, stop=True))
    add('5 %s split-K' % prec, prec, 70, 64, 544, 0.05,
        ('tiled', split, 'split-k', 'wide'), 'f32', eps[1],
        _options(hard=True, stop=True))
    add('5 %s three phases' % prec, prec, 45, 256, 384, 0.05,
        ('tiled', split, 'split-k', 'wide'), 'f32')
    add('5 %s past the streamed limit' % prec, prec, 8, 256, 16640, 0.03,
        ('tiled', split, 'split-k', 'wide'), 'f16x3')
    add('5 %s fused shape, early stopping' % prec, prec, 96, 256, 256, 0.05,
        ('tiled', split, 'single', 'wide'), 'f16x3', eps[2], ('stop',),
        eps=0.0)
  # 4 again (last, so that the seeds of the cases above stay): EpiProx behind
  # the 128 x 128 kernel, s % 4 != 0 past the cut-over
  add('4 f32 element s=201 past the cut-over', 'f32', CUT(201, 37), 100, 201,
      0.05, ('tiled', 'f32', 'single', 'element'), 'f32')
  return out


CASES = _cases()
BY_NAME = dict((c.name, c) for c in CASES)
REFUSALS = [('bf16', 8, 64, 64), ('bf16x3', 8, 16, 6)]
OPTIONS = [(c, o) for c in CASES for o in c.options]

Spec = collections.namedtuple(
    'Spec', 'variant threshold warm stop dev tile iters')


def option_spec(case, option):
  """An option is a few words: 'ista' / 'fista', a threshold of THRESHOLDS,
  'warm' (WARM_FROM float64 iterations give the start, WARM_ITERS more run),
  'stop' (ISTA under case.stop_eps), 'dev-eta' (the step size formed on the
  device) and 'tile' (the fused kernel's other MFMA tile).  The plain run of a
  case is the option 'fista'."""
  words = option.split()
  threshold = ([w for w in words if w in THRESHOLDS] or ['soft'])[0]
  stop, warm = 'stop' in words, 'warm' in words
  variant = 'ista' if ('ista' in words or stop) else 'fista'
  if stop:
    iters = STOP_ITERS
  elif warm:
    iters = WARM_ITERS
  elif 'hard' in threshold and case.route[1] == 'bf16x2':
    iters = HARD_ITERS_BF16X2
  elif 'hard' in threshold and case.route[1] == 'bf16':
    iters = HARD_ITERS_BF16
  else:
    iters = T
  return Spec(variant, threshold, warm, stop, 'dev-eta' in words,
              'tile' in words, iters)


def option_route(case, option, b, cus):
  """The route of a case under an option: an epsilon moves the on-chip shapes
  to the tiles, the forced tile is the other one."""
  spec = option_spec(case, option)
  route = fc_route(b, case.n, case.s, case.precision,
                   case.stop_eps if spec.stop else case.eps, spec.iters, cus)
  if spec.tile:
    assert route[0] == 'fused'
    route = route[:2] + (48 - route[2],)
  return route


def batch_size(case, cus):
  if isinstance(case.b, tuple):
    _, s, extra = case.b
    return ceil_div(16384 * cus, s) + extra
  return case.b


def auto_precision(case, cus):
  if case.auto != 'by-size':
    return case.auto
  return 'f16x3' if batch_size(case, cus) * case.s * case.n >= 240000000 else (
      'f32')


Problem = collections.namedtuple('Problem', 'case b X D eta rows')


@functools.lru_cache(maxsize=None)
def problem(name, cus):
  case = BY_NAME[name]
  seed = 9000 + 10 * CASES.index(case)
  b = batch_size(case, cus)
  X = helpers.gaussian_patches(seed, b, case.n)
  D = helpers.unit_rows(seed + 1, case.s, case.n)
  d64 = torch.from_numpy(D).double()
  eta = float(1. / sc_oracle.largest_eigenvalue(torch.mm(d64.t(), d64)))
  return Problem(case, b, X, D, eta, sample_rows(seed + 2, b))


def oracle(p, dtype, num_iters, variant='fista', rows=None, threshold='soft',
           **kw):
  X = p.X if rows is None else p.X[rows]
  nonneg, hard = THRESHOLDS[threshold]
  return sc_oracle.fc_ista_fista(
      torch.from_numpy(X).to(dtype), torch.from_numpy(p.D).to(dtype),
      p.case.lam, num_iters, variant=variant, stepsize=p.eta,
      nonnegative_only=nonneg, hard_threshold=hard, **kw)


# ------------------------------------------------- float64 iteration in numpy
def round_bf16(x):
  """float32(x) rounded to bf16, nearest even, as the (__bf16) conversions of
  csrc/split_operand.h and the pack kernels; returned as float64."""
  u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
  u = (u + (np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1)))) & (
      np.uint32(0xffff0000))
  return u.view(np.float32).astype(np.float64)


def shrink(pre, cutoff, threshold, fault=None):
  if fault == 'nonneg keeps negatives' and 'nonneg' in threshold:
    threshold = threshold[:-len('_nonneg')]
  if threshold == 'soft':
    return np.sign(pre) * np.maximum(np.abs(pre) - cutoff, 0.)
  if threshold == 'soft_nonneg':
    return np.maximum(pre - cutoff, 0.)
  keep = (np.abs(pre) if threshold == 'hard' else pre) >= cutoff
  if fault == 'hard subtracts the cutoff':
    return np.where(keep, pre - np.sign(pre) * cutoff, 0.)
  return np.where(keep, pre, 0.)


def _product(a, b, operands):
  """a @ b as a route forms it: None, exact; 'bf16', both operands rounded to
  bf16 first, the sum in float64, rounded to f32 once; 'bf16 f32', the same
  operands summed in float32 (numpy's order)."""
  if operands is None:
    return a @ b
  a, b = round_bf16(a), round_bf16(b)
  if operands == 'bf16':
    return (a @ b).astype(np.float32).astype(np.float64)
  assert operands == 'bf16 f32'
  return (a.astype(np.float32) @ b.astype(np.float32)).astype(np.float64)


def iterates(X, D, eta, lam, num_iters, variant='fista', threshold='soft',
             init=None, operands=None, fault=None):
  """ista_fista.py:100-146 in float64.  Returns (codes, pre-threshold values
  of every iteration).  fault: one of FAULTS, a kernel mistake that the gates
  of the route tests must notice."""
  X, D = X.astype(np.float64), D.astype(np.float64)
  cutoff = lam if fault == 'cutoff lam' else lam * eta
  betas = sc_oracle.fista_betas(num_iters + 1)
  if fault == 'momentum one ahead':
    betas = betas[1:]
  c = np.zeros((X.shape[0], D.shape[0])) if init is None else init.astype(
      np.float64)
  y = c
  if fault == 'warm start misses the evaluation point' and variant == 'fista':
    y = np.zeros_like(c)
  pres = []
  for k in range(num_iters):
    r = _product(y, D, operands) - X
    if operands is not None:        # R is an f32 array before it is packed
      r = r.astype(np.float32).astype(np.float64)
    pre = y - eta * _product(r, D.T, operands)
    new = shrink(pre, cutoff, threshold, fault)
    if k == num_iters - 1:
      if fault == 'stale column tile':
        new[:, 32:64] = c[:, 32:64]
      if fault == 'last rows from the row above':
        new[-5:] = new[-6:-1].copy()
    y = new + betas[k] * (new - c) if variant == 'fista' else new
    c = new
    pres.append(pre)
  return c, pres


FAULTS = ('momentum one ahead', 'cutoff lam', 'nonneg keeps negatives',
          'hard subtracts the cutoff', 'stale column tile',
          'last rows from the row above',
          'warm start misses the evaluation point')


def bf16_restatement(p, rows, spec, init=None, accumulate='f64'):
  """The iteration as the fused kernel's bf16 mode (NP = 1) runs it: Y and D,
  then R and D, rounded to bf16 on their way into the matrix cores, state and
  epilogue in higher precision.  accumulate='f64': products summed in float64
  and rounded to f32 once; 'f32': summed in float32."""
  return iterates(p.X[rows], p.D, p.eta, p.case.lam, spec.iters, spec.variant,
                  spec.threshold, init,
                  'bf16' if accumulate == 'f64' else 'bf16 f32')


def near_cutoff_rows(pres, cutoff, threshold, width):
  """Rows in which some pre-threshold value of some iteration lies within
  `width` of a hard threshold's cutoff."""
  near = np.zeros(pres[0].shape[0], bool)
  for pre in pres:
    mag = np.abs(pre) if threshold == 'hard' else pre
    near |= (np.abs(mag - cutoff) < width).any(axis=1)
  return near


# ----------------------------------------------------------------- references
# ref64 / ref32: the codes of `rows` (float64 oracle, float32 oracle; on a
# bf16 row the two restatements).  keep: the rows that meet the gate (all but
# those next to a hard threshold's cutoff).  init: the warm start of the whole
# batch.  count: iterations until early stopping.  gate: (rel, flip).
Ref = collections.namedtuple(
    'Ref', 'spec route rows ref64 ref32 keep init count gate distance')


def stop_count(p, dtype, eps):
  codes, trace = oracle(p, dtype, STOP_ITERS, 'ista',
                        early_stopping_epsilon=eps,
                        trace_at=set(range(1, STOP_ITERS + 1)))
  return codes.numpy(), len(trace)


def stop_count_numpy(p, eps, reduce=np.mean):
  """Iterations of ISTA under early stopping (ista_fista.py:135-144), with
  the reduction of |change| / eta as a parameter."""
  X, D = p.X.astype(np.float64), p.D.astype(np.float64)
  c = np.zeros((p.b, p.case.s))
  for k in range(STOP_ITERS):
    new = shrink(c - p.eta * ((c @ D - X) @ D.T), p.case.lam * p.eta, 'soft')
    change = reduce(np.abs(new - c) / p.eta)
    c = new
    if change < eps and k > 0:
      break
  return k + 1


@functools.lru_cache(maxsize=None)
def reference(name, cus, option='fista'):
  p = problem(name, cus)
  case = p.case
  spec = option_spec(case, option)
  route = option_route(case, option, p.b, cus)
  rows, init, init_rows, count, distance = p.rows, None, None, None, None
  if spec.warm:
    init = oracle(p, torch.float64, WARM_FROM,
                  threshold=spec.threshold).float().numpy()
    init_rows = init[rows]
  if spec.stop:
    # a mean over the whole batch: the oracle runs on all of it, and the count
    # must not hinge on a rounding
    rows = np.arange(p.b)
    ref64, count = stop_count(p, torch.float64, case.stop_eps)
    ref32, count32 = stop_count(p, torch.float32, case.stop_eps)
    assert 1 < count < STOP_ITERS, (name, count)
    assert count32 == count, (name, count32, count)
    for factor in (0.99, 1.01):
      assert stop_count(p, torch.float64, factor * case.stop_eps)[1] == (
          count), (name, factor)
  elif route[1] == 'bf16':
    ref64, pres = bf16_restatement(p, rows, spec, init_rows)
    ref32, _ = bf16_restatement(p, rows, spec, init_rows, accumulate='f32')
  else:
    kw = {} if init is None else {'initial_codes': init_rows}
    ref64, ref32 = [
        oracle(p, dtype, spec.iters, spec.variant, rows, spec.threshold,
               **dict((k, torch.from_numpy(v).to(dtype))
                      for k, v in kw.items())).numpy()
        for dtype in (torch.float64, torch.float32)]
  keep = np.ones(len(rows), bool)
  if 'hard' in spec.threshold:
    if route[1] != 'bf16':
      own, pres = iterates(p.X[rows], p.D, p.eta, case.lam, spec.iters,
                           spec.variant, spec.threshold, init_rows)
      assert np.array_equal(own != 0, ref64 != 0) and helpers.rel_err(
          own, ref64) < 1e-13, name
    keep = ~near_cutoff_rows(pres, case.lam * p.eta, spec.threshold,
                             NEAR_CUTOFF[route[1]])
  if route[1] == 'bf16':
    # The f32 accumulation of the kernel can carry an operand (Y or R of a
    # later iteration) across a bf16 boundary; how far that moves the codes is
    # measured between the float64-summed restatement and the float32-summed
    # one, and four times that distance (summation orders other than numpy's)
    # is the gate.  The l2 gate bounds a flipped entry by gate * |ref|, there
    # is no separate flip gate.
    # Under a hard threshold such a crossing is a jump of the cutoff's size in
    # whichever order it happens to occur, so no multiple of a measured
    # distance bounds it: those rows are shortened to one cold iteration, in
    # which both operands of both products are the inputs themselves and
    # nothing can cross; the distance is then that of the two summations alone.
    distance = helpers.rel_err(ref32[keep], ref64[keep])
    assert 'hard' not in spec.threshold or (spec.iters == 1 and init is None)
    the_gate = (4 * distance, float('inf'))
  else:
    the_gate = gate(route)
  return Ref(spec, route, rows, ref64, ref32, keep, init, count, the_gate,
             distance)


def active_fraction(codes):
  return float((np.asarray(codes) != 0).mean())


def assert_input_conditions(ref, what):
  """The case is not degenerate (a share of the codes is active, a share is
  not), float32 arithmetic reaches half the gate with no support flip above
  NEAR_THRESHOLD (the gate leaves room for the kernels' rounding and none for
  a wrong one), and a hard threshold leaves out few rows."""
  lo, hi = ACTIVE_BAND
  frac = active_fraction(ref.ref64[ref.keep])
  assert lo <= frac <= hi, '%s: %.3f of the codes active' % (what, frac)
  left_out = 1. - float(ref.keep.mean())
  assert left_out <= LEFT_OUT_CAP, '%s: %.3f of the rows left out' % (
      what, left_out)
  assert 'hard' in ref.spec.threshold or left_out == 0
  tol, flip = ref.gate
  if ref.route[1] == 'bf16':
    assert 0 < tol <= GATE_BF16_CAP, '%s: gate %.2e' % (what, tol)
    err = ref.distance
    assert err <= tol / 2
  else:
    err, _ = helpers.assert_codes_match(
        ref.ref32[ref.keep], ref.ref64[ref.keep], tol / 2,
        what + ': float32 oracle', max_flip_mag=helpers.NEAR_THRESHOLD)
  return frac, err, left_out
