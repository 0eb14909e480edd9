"""Cases, seeded inputs, float64 restatements, route mirrors and gates behind
tests/test_metrics_routes_gpu.py and tests/test_metrics_gates_host.py.

TrainingStep.compute_metrics (training/sparse_coding.py) is built from
vtc_row_stats, vtc_group_norm_sum, vtc_window_minmax, vtc_rows_mean_abs_diff
(csrc/metrics.hip), vtc_fc_residual (csrc/dict_update.hip), vtc_conv_residual
(csrc/conv.hip, launch_synthesis) and, for the step size, vtc_gram.  Every
case below names the route it must take and is the smallest shape that reaches
its branch.  Every restatement takes a `fault`: a numpy emulation of an edge
bug that the gate of the case must notice (FAULTS).  Nothing here needs a GPU.

Gates.  Counts, min / max and the zero of identical rows are exact.  The
reductions of non-negative terms have an a-priori float32 bound,
reduction_gate.  The contractions and the scalars of compute_metrics carry
measured gates (profiles/precision_metrics.txt)."""
import collections
import functools

import numpy as np
import torch

import helpers
import sc_oracle
from fc_routes_data import ceil_div, gemm_prefers_small

CUS = 256           # compute units of an MI355X: the routes the tables name
CUS_SMALLER = 64    # a part at which some of them differ (route_smaller)
STAT_THREADS = 256  # kStatThreads (csrc/metrics.hip)
MINMAX_BLOCKS = 512  # kMinMaxBlocks
UNIT = 2.0 ** -24   # unit roundoff of float32
EDGE_SHARE = 100    # an edge element carries this many gates of its row's sum


# ---------------------------------------------------------------------- gates
def reduction_gate(cols, own=0, divide=False):
  """Relative error bound of a block reduction of csrc/metrics.hip against the
  exact sum of its non-negative terms.  The order the kernel documents: thread
  t adds elements t, t + 256, ... in a chain of ceil(cols / 256) roundings (the
  fmaf of the sum of squares rounds once per link), the 64 lanes of a wave
  combine in a tree of 6 levels, and thread 0 adds the 4 wave partials in
  order.  A term therefore passes through at most
      k = own + ceil(cols / 256) + 6 + 4 (+ 1 for a final division)
  roundings, `own` being those of the term itself, and with non-negative terms
  the sum is off by at most (1 + u)^k - 1 <= 1.01 k u  (k u < 0.0099)."""
  k = own + ceil_div(cols, STAT_THREADS) + 6 + 4 + (1 if divide else 0)
  assert k * UNIT < 0.0099
  return 1.01 * k * UNIT


def group_gate(groups, m):
  """A group's term is sqrtf of a chain of m fmaf: (1 + u)^m under the root is
  m / 2 roundings, the root itself one, and one more in case the root is
  faithfully rather than correctly rounded."""
  return reduction_gate(groups, own=ceil_div(m, 2) + 2)


def diff_gate(cols):
  """|a - b|: one rounding of the difference; the mean divides once."""
  return reduction_gate(cols, own=1, divide=True)


# Relative l2 error against float64, per route: the largest error measured on
# an MI355X over the route's cases, times at most 3
# (profiles/precision_metrics.txt).
CONTRACTION_GATES = {
    'fc_residual gemm-small': 1.7e-7,   # measured 5.91e-8
    'fc_residual gemm-big': 7.5e-8,     # 2.55e-8
    'gram gemm-small': 5e-7,            # 1.77e-7
    'gram gemm-big': 3.4e-7,            # 1.14e-7
    'conv_residual unit': 6.5e-7,       # 2.27e-7
    'conv_residual plan': 6.5e-7,       # 2.18e-7
}
# the scalars of compute_metrics, per key, over the three modes
METRIC_GATES = {
    'Average LASSO L2 component': 2.8e-7,         # 9.40e-8
    'Average LASSO lagrange component': 3.2e-7,   # 1.08e-7
    'Average LASSO Loss': 1.6e-7,                 # 5.48e-8
    'Average Normalized L0': 6.9e-8,              # 2.33e-8
    'Average pSNR of reconstructions': 4.7e-7,    # 1.59e-7
    'Average change in dictionary kernels': 1.4e-7,   # 4.72e-8
}

FAULTS = ('drop last element', 'drop element 256', 'count -0.0',
          'flush subnormals', 'drop last group', 'read the frame',
          'drop last K quarter', 'drop last kernel chunk')


def _known(fault):
  assert fault is None or fault in FAULTS, fault


def rel(a, b):
  a = np.asarray(a, dtype=np.float64)
  b = np.asarray(b, dtype=np.float64)
  return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def worst_rel(a, b):
  """Largest relative error of an entry (reductions: one gate per row)."""
  a = np.asarray(a, dtype=np.float64).ravel()
  b = np.asarray(b, dtype=np.float64).ravel()
  return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


# -------------------------------------------------------------- route mirrors
def gemm_route(m, n, cus):
  """launch_gemm_f32 (csrc/gemm_f32.h), one slice, one batch entry, an
  element-wise epilogue."""
  return 'gemm-small' if gemm_prefers_small(m, n, cus) else 'gemm-big'


def unit_geometry(kh, kw, stride):
  """unit_geometry (csrc/conv_unit.h)."""
  return tuple(stride) == (1, 1) and kh == kw and kh in (5, 8, 11, 16)


def synthesis_chunk(kh, kw, stride, s):
  """s_chunk of plan_synthesis (csrc/conv.hip): kernels per LDS stage."""
  sv, sh = stride
  wy = 31 // sv + (kh - 1) // sv + 2
  wx = 31 // sh + (kw - 1) // sh + 2
  return max(1, min(s, (48 * 1024 // 4) // (wy * wx + kh * kw)))


def conv_route(kh, kw, stride, s):
  """launch_synthesis: ('unit',) or ('plan', s_chunk, kernels of the last
  chunk)."""
  if unit_geometry(kh, kw, stride):
    return ('unit',)
  chunk = synthesis_chunk(kh, kw, stride, s)
  return ('plan', chunk, s - chunk * (ceil_div(s, chunk) - 1))


def minmax_blocks(total):
  """Blocks of window_minmax_partial_kernel."""
  return min(MINMAX_BLOCKS, ceil_div(total, STAT_THREADS))


def edge_positions(cols):
  """First element, both sides of the first stride, last element."""
  return sorted(set(p for p in (0, STAT_THREADS - 1, STAT_THREADS, cols - 1)
                    if p < cols))


# ------------------------------------------------------------- vtc_row_stats
# kind 'codes': a sparse row; 'signed zeros': one that also holds -0.0 and
# float32 subnormals (torch.norm(p=0) counts the second and not the first)
RowStatsCase = collections.namedtuple('RowStatsCase', 'name rows cols kind')
ROW_STATS_CASES = (
    [RowStatsCase('cols=%d rows=%d' % (cols, rows), rows, cols, 'codes')
     for cols, rows in ((1, 1), (1, 3), (63, 3), (255, 3), (256, 3), (257, 1),
                        (257, 3), (1000, 3), (70001, 3))] +
    [RowStatsCase('signed zeros, subnormals cols=%d' % cols, 3, cols,
                  'signed zeros') for cols in (63, 600)])


def _weigh_edges(x, gate, rs):
  """Gives the edge elements of every row EDGE_SHARE gates (and a margin of
  2) of the row's sum of squares and of its l1 norm."""
  need = 2 * EDGE_SHARE * gate
  edges = edge_positions(x.shape[1])
  assert len(edges) * need < 0.5
  for row in x:
    row[edges] = 0.
    rest = row.astype(np.float64)
    room = 1. - len(edges) * need
    a = max(0.5, np.sqrt(need * (rest ** 2).sum() / room),
            need * np.abs(rest).sum() / room)
    row[edges] = a * np.where(rs.rand(len(edges)) < 0.5, -1., 1.)
  return x


@functools.lru_cache(maxsize=None)
def row_stats_input(case):
  rs = np.random.RandomState(1000 + ROW_STATS_CASES.index(case))
  shape = (case.rows, case.cols)
  x = np.where(rs.rand(*shape) < 0.4, 0.5 * rs.randn(*shape), 0.).astype(
      np.float32)        # (a product with the mask would leave -0.0 behind)
  if case.kind == 'signed zeros':
    pick = rs.rand(*shape)
    x[(x == 0) & (pick < 0.3)] = -0.0
    tiny = np.array([1e-40, -3e-42, 2.0 ** -149, -2.0 ** -127], np.float32)
    where = (x == 0) & (pick > 0.7)
    x[where] = tiny[rs.randint(0, len(tiny), int(where.sum()))]
    x[:, 1] = -0.0
    x[:, -2] = np.float32(2.0 ** -149)
  x = _weigh_edges(x, reduction_gate(case.cols), rs)
  x.setflags(write=False)
  return x


def _dropped(x, fault):
  """The columns an emulated reduction still reads."""
  _known(fault)
  keep = np.ones(x.shape[1], bool)
  if fault == 'drop last element':
    keep[-1] = False
  if fault == 'drop element 256':
    keep[STAT_THREADS] = False
  return x[:, keep]


def row_stats64(x, fault=None):
  """(sum of squares, l1, count of non-zeros) per row, in float64."""
  _known(fault)
  x32 = _dropped(np.asarray(x, dtype=np.float32), fault)
  x64 = x32.astype(np.float64)
  if fault == 'count -0.0':
    nonzero = x32.view(np.uint32) != 0
  elif fault == 'flush subnormals':
    nonzero = np.abs(x64) >= 2.0 ** -126
  else:
    nonzero = x64 != 0
  return ((x64 ** 2).sum(axis=1), np.abs(x64).sum(axis=1),
          nonzero.sum(axis=1).astype(np.float64))


def edge_shares(x):
  """Smallest share an edge element has of its row's sum of squares and l1."""
  x64 = np.asarray(x, dtype=np.float64)
  edges = edge_positions(x64.shape[1])
  sq = (x64[:, edges] ** 2) / (x64 ** 2).sum(axis=1, keepdims=True)
  ab = np.abs(x64[:, edges]) / np.abs(x64).sum(axis=1, keepdims=True)
  return float(min(sq.min(), ab.min()))


# -------------------------------------------------------- vtc_group_norm_sum
GroupCase = collections.namedtuple('GroupCase', 'name b s kind')
GROUP_CASES = [
    GroupCase('m=1, the l1 sum', 3, 300, 'singletons'),
    GroupCase('32 groups of 4', 3, 128, 'fours'),
    GroupCase('ragged 1 to 5', 3, 75, 'ragged'),
    GroupCase('overlapping groups', 3, 75, 'overlap'),
    GroupCase('700 groups', 2, 1400, 'many'),
]


def group_lists(case):
  if case.kind == 'singletons':
    return [[a] for a in range(case.s)]
  if case.kind == 'fours':
    return [list(range(4 * g, 4 * g + 4)) for g in range(case.s // 4)]
  if case.kind == 'many':    # 700 groups of 1, 2 or 3: 1400 atoms
    sizes = [1, 3, 2, 2] * 175
  else:                      # 25 groups of 1 to 5: 75 atoms
    sizes = [1, 5, 2, 4, 3] * 5
  rs = np.random.RandomState(7)
  order = rs.permutation(case.s)   # members are not neighbours in the row
  groups, at = [], 0
  for size in sizes:
    groups.append([int(a) for a in order[at:at + size]])
    at += size
  assert at == case.s
  if case.kind == 'overlap':       # atoms in two or three groups
    groups.insert(3, [groups[0][0], groups[1][0], groups[6][1]])
    groups.append([groups[0][0], groups[-1][-1], groups[2][0], groups[5][0]])
  return groups


@functools.lru_cache(maxsize=None)
def group_input(case):
  """Codes whose second row is all zero (the last row where b = 2)."""
  rs = np.random.RandomState(2000 + GROUP_CASES.index(case))
  shape = (case.b, case.s)
  codes = (0.5 * rs.randn(*shape) * (rs.rand(*shape) < 0.6)).astype(np.float32)
  groups = group_lists(case)
  for g in (groups[0], groups[-1]):
    codes[:, g] = np.where(rs.rand(case.b, len(g)) < 0.5, -1., 1.) * 0.7
  codes[1] = 0.
  codes.setflags(write=False)
  return codes


def group_norm_sum64(codes, groups, fault=None):
  _known(fault)
  c = np.asarray(codes, dtype=np.float32).astype(np.float64)
  if fault == 'drop last group':
    groups = groups[:-1]
  return sum(np.sqrt((c[:, g] ** 2).sum(axis=1)) for g in groups)


def group_shares(codes, groups):
  """Smallest share the first and the last group have of a non-zero row."""
  c = np.asarray(codes, dtype=np.float64)
  total = group_norm_sum64(codes, groups)
  live = total > 0
  return float(min((np.sqrt((c[:, g] ** 2).sum(axis=1))[live] /
                    total[live]).min() for g in (groups[0], groups[-1])))


# --------------------------------------------------------- vtc_window_minmax
# pad None: the (1, b, n) window of the fully-connected path, outer pitch 0.
# Else (outer, h, w) planes whose frame holds +-1000 and the window of the
# convolutional path: outer_pitch h * w, row_pitch w, the pointer moved by the
# leading pad.  kind: 'random'; 'max first, min last' / 'min first, max last'
# element of the window; 'negative'; 'equal'.
WindowCase = collections.namedtuple('WindowCase',
                                    'name outer h w pad kind blocks')
_PAD = ((6, 5), (4, 6))
WINDOW_CASES = [
    WindowCase('fc plain 37 x 300', 1, 37, 300, None, 'random', 44),
    WindowCase('fc plain, max first', 1, 37, 300, None, 'max first, min last',
               44),
    WindowCase('fc plain one element', 1, 1, 1, None, 'random', 1),
    WindowCase('cropped 6 x 45 x 52', 6, 45, 52, _PAD, 'random', 34),
    WindowCase('cropped, max first', 6, 45, 52, _PAD, 'max first, min last',
               34),
    WindowCase('cropped, min first', 6, 45, 52, _PAD, 'min first, max last',
               34),
    WindowCase('cropped, all negative', 6, 45, 52, _PAD, 'negative', 34),
    WindowCase('cropped, all equal', 6, 45, 52, _PAD, 'equal', 34),
    WindowCase('capped 3 x 250 x 211', 3, 255, 220, ((2, 3), (5, 4)),
               'random', 512),
    WindowCase('capped, min first', 3, 255, 220, ((2, 3), (5, 4)),
               'min first, max last', 512),
    WindowCase('capped plain, max first', 1, 515, 300, None,
               'max first, min last', 512),
]

Window = collections.namedtuple(
    'Window', 'buffer offset outer rows cols outer_pitch row_pitch crop')


@functools.lru_cache(maxsize=None)
def window_input(case):
  rs = np.random.RandomState(3000 + WINDOW_CASES.index(case))
  (lv, tv), (lh, th) = case.pad if case.pad is not None else ((0, 0), (0, 0))
  buf = np.where(rs.rand(case.outer, case.h, case.w) < 0.5, -1000.,
                 1000.).astype(np.float32)
  ih, iw = case.h - lv - tv, case.w - lh - th
  win = rs.randn(case.outer, ih, iw).astype(np.float32)
  if case.kind == 'negative':
    win = -np.abs(win) - 1
  elif case.kind == 'equal':
    win[:] = 0.75
  elif case.kind != 'random':
    hi, lo = (0, -1) if case.kind == 'max first, min last' else (-1, 0)
    win.reshape(-1)[hi] = 50.
    win.reshape(-1)[lo] = -50.
  buf[:, lv:lv + ih, lh:lh + iw] = win
  buf.setflags(write=False)
  if case.pad is None:
    assert case.outer == 1
    return Window(buf.reshape(-1), 0, 1, case.h, case.w, 0, case.w, win)
  return Window(buf.reshape(-1), lv * case.w + lh, case.outer, ih, iw,
                case.h * case.w, case.w, win)


def window_minmax64(w, fault=None):
  """min and max of element (o, r, c) at
  buffer[offset + o * outer_pitch + r * row_pitch + c]."""
  _known(fault)
  if fault == 'read the frame':
    return float(w.buffer.min()), float(w.buffer.max())
  index = (w.offset + np.arange(w.outer)[:, None, None] * w.outer_pitch +
           np.arange(w.rows)[None, :, None] * w.row_pitch +
           np.arange(w.cols)[None, None, :])
  values = w.buffer[index]
  return float(values.min()), float(values.max())


# ---------------------------------------------------- vtc_rows_mean_abs_diff
DiffCase = collections.namedtuple('DiffCase', 'name rows cols')
DIFF_CASES = [DiffCase('cols=%d' % cols, 5, cols)
              for cols in (1, 121, 257, 768)]
IDENTICAL_ROW = 2


@functools.lru_cache(maxsize=None)
def diff_input(case):
  """(a, b): b a perturbed a, row IDENTICAL_ROW the same in both; the edge
  elements differ by about the largest difference of the row."""
  rs = np.random.RandomState(4000 + DIFF_CASES.index(case))
  a = rs.randn(case.rows, case.cols).astype(np.float32)
  b = (a + 0.01 * rs.randn(case.rows, case.cols)).astype(np.float32)
  edges = edge_positions(case.cols)
  b[:, edges] = a[:, edges] + np.float32(0.03)
  b[IDENTICAL_ROW] = a[IDENTICAL_ROW]
  a.setflags(write=False)
  b.setflags(write=False)
  return a, b


def rows_mean_abs_diff64(a, b, fault=None):
  cols = np.asarray(a).shape[1]
  d = np.abs(np.asarray(a, dtype=np.float32).astype(np.float64) -
             np.asarray(b, dtype=np.float32).astype(np.float64))
  return _dropped(d, fault).sum(axis=1) / cols


def diff_shares(a, b):
  d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
  live = d.sum(axis=1) > 0
  return float((d[live][:, edge_positions(d.shape[1])] /
                d[live].sum(axis=1, keepdims=True)).min())


# ------------------------------------------------- vtc_fc_residual, vtc_gram
def small_k_quarter(k):
  """K range of a wave of gemm_f32_small_kernel: four quarters, each a multiple
  of 16 long."""
  return ceil_div(k, 64) * 16


def product64(a, b, fault=None):
  """a (M, K) times b (K, N) in float64; the emulation leaves out the last
  quarter of K that holds anything."""
  _known(fault)
  a = np.asarray(a, dtype=np.float32).astype(np.float64)
  b = np.asarray(b, dtype=np.float32).astype(np.float64)
  if fault == 'drop last K quarter':
    k = a.shape[1]
    quarter = small_k_quarter(k)
    keep = quarter * (ceil_div(k, quarter) - 1)
    return a[:, :keep] @ b[:keep]
  return a @ b


# route: at CUS compute units; route_smaller: at CUS_SMALLER
FcCase = collections.namedtuple('FcCase', 'name b n s route route_smaller')


def _fc_case(b, n, s, route='gemm-small', smaller=None):
  return FcCase('b=%d n=%d s=%d' % (b, n, s), b, n, s, route,
                smaller or route)


FC_RESIDUAL_CASES = [
    # K = s against the K quarters of 16; n and s no multiples of 4
    _fc_case(37, 33, 1), _fc_case(37, 31, 15), _fc_case(1, 33, 17),
    _fc_case(37, 300, 63), _fc_case(37, 1, 65), _fc_case(37, 300, 1030),
    _fc_case(1, 1, 1),
    # 16-byte loads of the codes: s a multiple of 4
    _fc_case(37, 32, 64), _fc_case(37, 300, 1028),
    # small on 256 compute units, 128 x 128 tiles on 64
    _fc_case(600, 2052, 17, smaller='gemm-big'),
    # b n just above 16384 x 256 and more than 8 tiles
    _fc_case(2100, 2052, 64, 'gemm-big'),
]


@functools.lru_cache(maxsize=None)
def fc_residual_input(case):
  """(X, D, C): codes random and sparse, not fitted, so that the residual is
  of the order of X."""
  seed = 5000 + 3 * FC_RESIDUAL_CASES.index(case)
  rs = np.random.RandomState(seed)
  X = helpers.gaussian_patches(seed + 1, case.b, case.n)
  D = helpers.unit_rows(seed + 2, case.s, case.n)
  density = 0.2 if case.s > 20 else 0.7
  C = (0.05 * rs.randn(case.b, case.s) *
       (rs.rand(case.b, case.s) < density)).astype(np.float32)
  C[:, -1] = 0.05        # the last k of every row is live
  return X, D, C


def fc_residual64(X, D, C, fault=None):
  return product64(C, D, fault) - np.asarray(X, dtype=np.float64)


GramCase = collections.namedtuple(
    'GramCase', 'name rows cols transpose_a route route_smaller')


def _gram_case(rows, cols, transpose_a, route='gemm-small', smaller=None):
  return GramCase('%d x %d %s' % (rows, cols, 'A^T A' if transpose_a else
                                  'A A^T'), rows, cols, transpose_a, route,
                  smaller or route)


GRAM_CASES = [
    _gram_case(75, 15, 1), _gram_case(128, 121, 1), _gram_case(1030, 300, 1),
    _gram_case(40, 2052, 1, 'gemm-big'),
    _gram_case(75, 15, 0), _gram_case(128, 121, 0),
    _gram_case(1030, 300, 0, smaller='gemm-big'),
    _gram_case(2052, 40, 0, 'gemm-big'),
]


def gram_shape(case):
  """(M = N, K) of the product."""
  return ((case.cols, case.rows) if case.transpose_a else
          (case.rows, case.cols))


@functools.lru_cache(maxsize=None)
def gram_input(case):
  return helpers.unit_rows(6000 + GRAM_CASES.index(case), case.rows,
                           case.cols)


def gram64(a, transpose_a, fault=None):
  a = np.asarray(a, dtype=np.float32)
  return product64(a.T, a, fault) if transpose_a else product64(a, a.T, fault)


# --------------------------------------------------------- vtc_conv_residual
# ch, cw: the code map; the padded image is (ch - 1) * stride + kernel.  pad:
# None, or ((lead_v, trail_v), (lead_h, trail_h)); a trailing 0 blanks the
# axis as the reference's `-0:` slice does (utils/convolutions.py:17-24).
ConvCase = collections.namedtuple(
    'ConvCase', 'name c kh kw stride s b ch cw pad route')
CONV_CASES = [
    ConvCase('unit 11x11 c=1, symmetric pad', 1, 11, 11, (1, 1), 9, 2, 27, 40,
             ((10, 10), (10, 10)), ('unit',)),
    ConvCase('unit 5x5 c=3, asymmetric pad', 3, 5, 5, (1, 1), 13, 2, 30, 37,
             ((4, 3), (2, 4)), ('unit',)),
    ConvCase('unit 5x5 c=3, no pad', 3, 5, 5, (1, 1), 13, 2, 30, 37, None,
             ('unit',)),
    ConvCase('strided 8x8 stride 4, no pad', 1, 8, 8, (4, 4), 6, 3, 9, 12,
             None, ('plan', 6, 6)),
    ConvCase('strided 8x8 stride 4, symmetric pad', 1, 8, 8, (4, 4), 6, 3, 9,
             12, ((4, 4), (4, 4)), ('plan', 6, 6)),
    ConvCase('strided 8x8 stride 4 c=2, trailing 0', 2, 8, 8, (4, 4), 6, 2, 9,
             12, ((4, 0), (4, 4)), ('plan', 6, 6)),
    ConvCase('6x9 stride (2, 3) c=2, asymmetric pad', 2, 6, 9, (2, 3), 11, 2,
             15, 11, ((4, 5), (6, 7)), ('plan', 11, 11)),
    ConvCase('7x7 stride 1 s=20, three chunks', 1, 7, 7, (1, 1), 20, 2, 39, 46,
             ((6, 5), (4, 6)), ('plan', 7, 6)),
]


def conv_image_shape(case):
  return ((case.ch - 1) * case.stride[0] + case.kh,
          (case.cw - 1) * case.stride[1] + case.kw)


@functools.lru_cache(maxsize=None)
def conv_input(case):
  """(images, kernels, codes): the frame of the images holds data too, so a
  mask that is off by one shows."""
  rs = np.random.RandomState(7000 + CONV_CASES.index(case))
  height, width = conv_image_shape(case)
  x = (0.5 * rs.randn(case.b, case.c, height, width)).astype(np.float32)
  d = rs.randn(case.s, case.c, case.kh, case.kw).astype(np.float32)
  d /= np.sqrt((d.astype(np.float64) ** 2).sum(axis=(1, 2, 3)))[
      :, None, None, None].astype(np.float32)
  shape = (case.b, case.s, case.ch, case.cw)
  codes = (0.5 * rs.randn(*shape) * (rs.rand(*shape) < 0.2)).astype(
      np.float32)
  codes[:, -1, -1, -1] = 0.5    # the last kernel reaches the last pixel
  return x, d, codes


def conv_residual64(x, d, codes, stride, pad, fault=None, chunk=None):
  """conv_transpose2d of the codes, minus the images, times
  sc_oracle.conv_mask, as update_oracle.conv_gradient_sum forms it."""
  _known(fault)
  x = torch.as_tensor(x).double()
  d = torch.as_tensor(d).double()
  codes = torch.as_tensor(codes).double()
  if fault == 'drop last kernel chunk':
    keep = chunk * (ceil_div(d.shape[0], chunk) - 1)
    d, codes = d[:keep], codes[:, :keep]
  if d.shape[0]:
    recon = sc_oracle.conv_synthesis(codes, d, stride)
  else:
    recon = torch.zeros_like(x)
  return (sc_oracle.conv_mask(x, pad) * (recon - x)).numpy()


# ------------------------------------------------------------ compute_metrics
METRIC_KEYS = sorted(METRIC_GATES)
EXACT_ROW = 1           # the row whose reconstruction is exact: mse == 0
SPARSITY_WEIGHT = 0.05
METRIC_MODES = ('fc', 'sub', 'conv')


def metrics_params(mode):
  """all_params of a TrainingStep that only runs compute_metrics."""
  if mode == 'conv':
    return {'mode': 'convolutional', 'code_inference_algorithm': 'fista',
            'dictionary_update_algorithm': 'sc_steepest_descent',
            'strides': (1, 1), 'padding': ((6, 5), (4, 6))}
  params = {'mode': 'fully-connected', 'code_inference_algorithm': 'fista',
            'dictionary_update_algorithm': 'sc_steepest_descent'}
  if mode == 'sub':
    # 206 groups of 3 to 7 over the 1030 atoms
    sizes = ([3, 7, 5, 4, 6] * 42)[:205] + [5]
    order = np.random.RandomState(11).permutation(1030)
    bounds = np.cumsum([0] + sizes)
    assert bounds[-1] == 1030 and len(sizes) == 206
    params.update({
        'code_inference_algorithm': 'subspace_fista',
        'dictionary_update_algorithm': 'subspace_sc_cheap_quadratic_descent',
        'group_assignments': [
            [int(a) for a in order[bounds[i]:bounds[i + 1]]]
            for i in range(206)],
        'subspace_alignment_penalty': 2e-4})
  return params


@functools.lru_cache(maxsize=None)
def metrics_problem(mode):
  """(images, codes, dictionary, previous dictionary), float32, past one
  stride of every reduction.  Row EXACT_ROW is twice one atom, coded by that
  atom alone: float32 and float64 both reconstruct it exactly."""
  rs = np.random.RandomState(8000 + METRIC_MODES.index(mode))
  if mode == 'conv':
    b, c, height, width, s, k = 3, 3, 45, 52, 20, 7
    (lv, tv), (lh, th) = metrics_params(mode)['padding']
    x = np.where(rs.rand(b, c, height, width) < 0.5, -9., 9.).astype(
        np.float32)        # the frame: outside the signal range
    x[:, :, lv:height - tv, lh:width - th] = 0.5 * rs.randn(
        b, c, height - lv - tv, width - lh - th)
    d = rs.randn(s, c, k, k).astype(np.float32)
    d /= np.sqrt((d.astype(np.float64) ** 2).sum(axis=(1, 2, 3)))[
        :, None, None, None].astype(np.float32)
    shape = (b, s, height - k + 1, width - k + 1)
    codes = (0.3 * rs.randn(*shape) * (rs.rand(*shape) < 0.05)).astype(
        np.float32)
    # the exact row: kernel 5 at code position (10, 12), inside the window
    codes[EXACT_ROW] = 0.
    codes[EXACT_ROW, 5, 10, 12] = 2.
    x[EXACT_ROW, :, lv:height - tv, lh:width - th] = 0.
    x[EXACT_ROW, :, 10:10 + k, 12:12 + k] = 2 * d[5]
    assert 10 >= lv and 10 + k <= height - tv
    assert 12 >= lh and 12 + k <= width - th
  else:
    b, n, s = 37, 300, 1030
    x = helpers.gaussian_patches(8100, b, n)
    d = helpers.unit_rows(8101, s, n)
    codes = (0.05 * rs.randn(b, s) * (rs.rand(b, s) < 0.2)).astype(np.float32)
    codes[EXACT_ROW] = 0.
    codes[EXACT_ROW, 700] = 2.
    x[EXACT_ROW] = 2 * d[700]
  previous = (d + 1e-3 * rs.randn(*d.shape)).astype(np.float32)
  return x, codes, d, previous


def metrics64(mode, images, codes, dictionary, previous, sparsity_weight,
              params):
  """TrainingStep.compute_metrics composed from the float64 restatements of
  the entry points, call for call."""
  x = np.asarray(images, dtype=np.float32)
  c = np.asarray(codes, dtype=np.float32)
  d = np.asarray(dictionary, dtype=np.float32)
  b = x.shape[0]
  if mode == 'conv':
    pad = params['padding']
    residual = conv_residual64(x, d, c, params['strides'], pad)
    _, chans, h, w = x.shape
    (lv, tv), (lh, th) = pad if pad is not None else ((0, 0), (0, 0))
    ih, iw = h - lv - tv, w - lh - th
    pixels = chans * ih * iw
    lo, hi = window_minmax64(Window(x.reshape(-1), lv * w + lh, b * chans, ih,
                                    iw, h * w, w, None))
  else:
    residual = fc_residual64(x, d, c)
    pixels = x.shape[1]
    lo, hi = window_minmax64(Window(x.reshape(-1), 0, 1, b, x.shape[1], 0,
                                    x.shape[1], None))
  sq_err, _, _ = row_stats64_exact(residual.reshape(b, -1))
  code_rows = c.reshape(b, -1)
  _, l1, l0 = row_stats64(code_rows)
  if mode == 'sub':
    lagrange = group_norm_sum64(c, params['group_assignments'])
  else:
    lagrange = l1
  out = {}
  out['Average LASSO L2 component'] = np.mean(0.5 * sq_err)
  out['Average LASSO lagrange component'] = np.mean(sparsity_weight * lagrange)
  out['Average LASSO Loss'] = (out['Average LASSO L2 component'] +
                               out['Average LASSO lagrange component'])
  out['Average Normalized L0'] = float(np.mean(l0 / code_rows.shape[1]))
  mse = sq_err / pixels
  out['Average pSNR of reconstructions'] = np.mean(
      10. * np.log10((hi - lo) ** 2 / mse[mse != 0]))
  out['Average change in dictionary kernels'] = rows_mean_abs_diff64_exact(
      d.reshape(d.shape[0], -1),
      np.asarray(previous, np.float64).reshape(d.shape[0], -1))
  return out


def row_stats64_exact(x64):
  """row_stats64 of values that are float64 already (a float64 residual)."""
  x64 = np.asarray(x64, dtype=np.float64)
  return ((x64 ** 2).sum(axis=1), np.abs(x64).sum(axis=1),
          (x64 != 0).sum(axis=1).astype(np.float64))


def rows_mean_abs_diff64_exact(a64, b64):
  return np.abs(np.asarray(a64, np.float64) -
                np.asarray(b64, np.float64)).mean(axis=1)


def oracle_metrics(mode, images, codes, dictionary, previous, sparsity_weight,
                   params):
  """sc_oracle.compute_metrics evaluated on float64 tensors."""
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
  return sc_oracle.compute_metrics(t(images), t(codes), t(dictionary),
                                   t(previous), sparsity_weight, params)


def metric_errors(got, want):
  """Relative l2 error per key (the scalars: relative error)."""
  assert sorted(got) == sorted(want) == METRIC_KEYS
  return dict((key, rel(got[key], want[key])) for key in METRIC_KEYS)
