"""The validation metrics and the C entry points they are built from, against
float64.

TrainingStep.compute_metrics (training/sparse_coding.py) calls vtc_row_stats,
vtc_group_norm_sum, vtc_window_minmax, vtc_rows_mean_abs_diff,
vtc_fc_residual and vtc_conv_residual; every step size comes from vtc_gram.
One table of cases per entry point (tests/metrics_data.py) names the route a
case must take; the Python mirrors of the C dispatch assert it with the
device's CU count, so a dispatch change fails here instead of quietly moving
coverage.  Per case: the C ABI result against its float64 restatement, two
runs bit for bit, one report line.  Counts, min / max and the zero of
identical rows are exact; the reductions meet the a-priori float32 bound of
their summation order; the contractions and the scalars of compute_metrics
meet measured gates (profiles/precision_metrics.txt).
tests/test_metrics_gates_host.py shows what each gate catches."""
import ctypes
import time

import numpy as np
import pytest
import torch

import helpers
import metrics_data as md

pytestmark = pytest.mark.gpu

CANARY = 1234.5


@pytest.fixture(scope='module', autouse=True)
def _module_time():
  start = time.perf_counter()
  yield
  print('tests/test_metrics_routes_gpu.py: %.1f s' % (
      time.perf_counter() - start))


def _cus():
  return torch.cuda.get_device_properties(0).multi_processor_count


def _lib():
  import vtc_hip
  return vtc_hip, vtc_hip.load_library()


def _report(name, route, **figures):
  print('%-44s %-22s %s' % (name, route, '  '.join(
      '%s %.2e' % kv for kv in sorted(figures.items()))))


def _dev(a, device):
  """A copy on the device (the cached inputs are read-only arrays)."""
  return helpers.to_dev(np.array(a), device)


def _canaries(count, device):
  return torch.full((count,), CANARY, dtype=torch.float32, device=device)


def _twice(run):
  first, second = run(), run()
  for a, b in zip(first, second):
    assert torch.equal(a, b), 'two runs differ'
  return [t.cpu().numpy() for t in first]


# ------------------------------------------------------------- vtc_row_stats
def _row_stats(x, want=(True, True, True)):
  vtc_hip, lib = _lib()
  rows, cols = x.shape
  outs = [_canaries(rows, x.device) if w else None for w in want]
  vtc_hip.check(lib.vtc_row_stats(
      vtc_hip.ptr(x), rows, cols, vtc_hip.ptr(outs[0]), vtc_hip.ptr(outs[1]),
      vtc_hip.ptr(outs[2]), vtc_hip.current_stream(x.device)),
      'vtc_row_stats')
  return outs


@pytest.mark.parametrize('case', md.ROW_STATS_CASES,
                         ids=[c.name for c in md.ROW_STATS_CASES])
def test_row_stats(device, case):
  """Sum of squares and l1 within the bound of the summation order, the count
  of non-zeros exact (-0.0 is none, a subnormal is one), each output null in
  turn."""
  x = md.row_stats_input(case)
  X = _dev(x, device)
  sumsq, l1, l0 = _twice(lambda: _row_stats(X))
  ref_sq, ref_l1, ref_l0 = md.row_stats64(x)
  gate = md.reduction_gate(case.cols)
  errs = {'sumsq': md.worst_rel(sumsq, ref_sq), 'l1': md.worst_rel(l1, ref_l1)}
  _report(case.name, 'stride x %d' % md.ceil_div(case.cols, md.STAT_THREADS),
          gate=gate, l0_diff=float(np.abs(l0 - ref_l0).max()), **errs)
  assert np.array_equal(l0.astype(np.float64), ref_l0)
  assert errs['sumsq'] < gate and errs['l1'] < gate
  full = [sumsq, l1, l0]
  for absent in range(3):
    want = tuple(i != absent for i in range(3))
    outs = _row_stats(X, want)
    for i in range(3):
      if want[i]:
        assert np.array_equal(outs[i].cpu().numpy(), full[i]), (absent, i)


# -------------------------------------------------------- vtc_group_norm_sum
def _group_norm_sum(C, tables):
  vtc_hip, lib = _lib()
  b, s = C.shape
  out = _canaries(b, C.device)
  vtc_hip.check(lib.vtc_group_norm_sum(
      vtc_hip.ptr(C), vtc_hip.ptr(tables.index), vtc_hip.ptr(tables.valid),
      vtc_hip.ptr(out), b, s, tables.num_groups, tables.m,
      vtc_hip.current_stream(C.device)), 'vtc_group_norm_sum')
  return [out]


@pytest.mark.parametrize('case', md.GROUP_CASES,
                         ids=[c.name for c in md.GROUP_CASES])
def test_group_norm_sum(device, case):
  """Sum of the group norms on the tables of vtc_hip.groups.tables_for; an
  all-zero row gives 0, groups of one give the l1 sum of vtc_row_stats bit for
  bit (the same terms in the same order)."""
  from vtc_hip import groups as group_tables
  codes, groups = md.group_input(case), md.group_lists(case)
  C = _dev(codes, device)
  tables = group_tables.tables_for(groups, case.s, device)
  assert tables.num_groups == len(groups)
  assert tables.m == max(len(g) for g in groups)
  got, = _twice(lambda: _group_norm_sum(C, tables))
  ref = md.group_norm_sum64(codes, groups)
  gate = md.group_gate(len(groups), tables.m)
  live = ref > 0
  err = md.worst_rel(got[live], ref[live])
  _report(case.name, '%d groups, m=%d' % (len(groups), tables.m), gate=gate,
          err=err)
  assert not live[1] and got[1] == 0
  assert err < gate
  if case.kind == 'singletons':
    l1 = _row_stats(C, (False, True, False))[1].cpu().numpy()
    assert np.array_equal(got, l1)


# --------------------------------------------------------- vtc_window_minmax
def _window_minmax(buf, w):
  vtc_hip, lib = _lib()
  device = buf.device
  ws = vtc_hip.workspace(lib.vtc_window_minmax_workspace_bytes(), device)
  out = _canaries(2, device)
  vtc_hip.check(lib.vtc_window_minmax(
      vtc_hip.ptr(buf[w.offset:]), w.outer, w.rows, w.cols, w.outer_pitch,
      w.row_pitch, vtc_hip.ptr(out), vtc_hip.ptr(ws), ws.numel(),
      vtc_hip.current_stream(device)), 'vtc_window_minmax')
  return [out]


@pytest.mark.parametrize('case', md.WINDOW_CASES,
                         ids=[c.name for c in md.WINDOW_CASES])
def test_window_minmax(device, case):
  """min and max of the window, exact; the frame around a cropped window holds
  +-1000 and is not read."""
  w = md.window_input(case)
  assert md.minmax_blocks(w.outer * w.rows * w.cols) == case.blocks
  buf = _dev(w.buffer, device)
  got, = _twice(lambda: _window_minmax(buf, w))
  lo, hi = md.window_minmax64(w)
  _report(case.name, '%d blocks' % case.blocks, min_diff=abs(got[0] - lo),
          max_diff=abs(got[1] - hi))
  assert float(got[0]) == lo and float(got[1]) == hi


# ---------------------------------------------------- vtc_rows_mean_abs_diff
def _rows_mean_abs_diff(A, B):
  vtc_hip, lib = _lib()
  rows, cols = A.shape
  out = _canaries(rows, A.device)
  vtc_hip.check(lib.vtc_rows_mean_abs_diff(
      vtc_hip.ptr(A), vtc_hip.ptr(B), rows, cols, vtc_hip.ptr(out),
      vtc_hip.current_stream(A.device)), 'vtc_rows_mean_abs_diff')
  return [out]


@pytest.mark.parametrize('case', md.DIFF_CASES,
                         ids=[c.name for c in md.DIFF_CASES])
def test_rows_mean_abs_diff(device, case):
  a, b = md.diff_input(case)
  A, B = _dev(a, device), _dev(b, device)
  got, = _twice(lambda: _rows_mean_abs_diff(A, B))
  ref = md.rows_mean_abs_diff64(a, b)
  gate = md.diff_gate(case.cols)
  live = np.arange(case.rows) != md.IDENTICAL_ROW
  err = md.worst_rel(got[live], ref[live])
  _report(case.name, 'stride x %d' % md.ceil_div(case.cols, md.STAT_THREADS),
          gate=gate, err=err)
  assert got[md.IDENTICAL_ROW] == 0 and ref[md.IDENTICAL_ROW] == 0
  assert err < gate


# ----------------------------------------------------------- vtc_fc_residual
def _fc_residual(X, D, C):
  vtc_hip, lib = _lib()
  b, n = X.shape
  out = _canaries(b * n, X.device).view(b, n)
  vtc_hip.check(lib.vtc_fc_residual(
      vtc_hip.ptr(X), vtc_hip.ptr(D), vtc_hip.ptr(C), vtc_hip.ptr(out), b, n,
      D.shape[0], vtc_hip.current_stream(X.device)), 'vtc_fc_residual')
  return [out]


@pytest.mark.parametrize('case', md.FC_RESIDUAL_CASES,
                         ids=[c.name for c in md.FC_RESIDUAL_CASES])
def test_fc_residual(device, case):
  """C D - X on the 32 x 32-tile kernel at every K-quarter edge and on the
  128 x 128 tiles."""
  assert md.gemm_route(case.b, case.n, _cus()) == case.route
  x, d, c = md.fc_residual_input(case)
  X, D, C = (_dev(a, device) for a in (x, d, c))
  got, = _twice(lambda: _fc_residual(X, D, C))
  ref = md.fc_residual64(x, d, c)
  err = md.rel(got, ref)
  gate = md.CONTRACTION_GATES['fc_residual ' + case.route]
  _report(case.name, case.route, err=err, gate=gate,
          size=float(np.linalg.norm(ref) / np.linalg.norm(x)))
  assert np.isfinite(got).all()
  assert err < gate


def test_fc_residual_empty_batch(device):
  """b = 0 returns VTC_OK and writes nothing."""
  vtc_hip, lib = _lib()
  D = _dev(helpers.unit_rows(1, 17, 33), device)
  out = _canaries(64, device)
  status = lib.vtc_fc_residual(
      vtc_hip.ptr(D), vtc_hip.ptr(D), vtc_hip.ptr(D), vtc_hip.ptr(out), 0, 33,
      17, vtc_hip.current_stream(device))
  assert status == vtc_hip.OK
  assert bool((out == CANARY).all())


# ------------------------------------------------------------------ vtc_gram
def _gram(A, transpose_a):
  vtc_hip, lib = _lib()
  rows, cols = A.shape
  side = cols if transpose_a else rows
  out = _canaries(side * side, A.device).view(side, side)
  vtc_hip.check(lib.vtc_gram(
      vtc_hip.ptr(A), rows, cols, transpose_a, vtc_hip.ptr(out),
      vtc_hip.current_stream(A.device)), 'vtc_gram')
  return [out]


@pytest.mark.parametrize('case', md.GRAM_CASES,
                         ids=[c.name for c in md.GRAM_CASES])
def test_gram(device, case):
  """A^T A and A A^T on both kernels, against float64 and against the
  result's own transpose."""
  side, _ = md.gram_shape(case)
  assert md.gemm_route(side, side, _cus()) == case.route
  a = md.gram_input(case)
  A = _dev(a, device)
  got, = _twice(lambda: _gram(A, case.transpose_a))
  assert got.shape == (side, side)
  err = md.rel(got, md.gram64(a, case.transpose_a))
  sym = md.rel(got, got.T)
  gate = md.CONTRACTION_GATES['gram ' + case.route]
  _report(case.name, case.route, err=err, symmetry=sym, gate=gate)
  assert err < gate and sym < gate


# --------------------------------------------------------- vtc_conv_residual
def _conv_residual(X, D, C, geom):
  vtc_hip, lib = _lib()
  out = _canaries(X.numel(), X.device).view(X.shape)
  vtc_hip.check(lib.vtc_conv_residual(
      vtc_hip.ptr(X), vtc_hip.ptr(D), vtc_hip.ptr(C), vtc_hip.ptr(out),
      ctypes.byref(geom), vtc_hip.current_stream(X.device)),
      'vtc_conv_residual')
  return [out]


@pytest.mark.parametrize('case', md.CONV_CASES,
                         ids=[c.name for c in md.CONV_CASES])
def test_conv_residual(device, case):
  """mask * (synthesis - images) on the stride-1 kernel and on the strided
  plan, one and several chunks of kernels, every kind of mask."""
  from utils import convolutions
  assert md.conv_route(case.kh, case.kw, case.stride, case.s) == case.route
  x, d, c = md.conv_input(case)
  X, D, C = (_dev(a, device) for a in (x, d, c))
  geom = convolutions.geometry(X, D, case.stride, case.pad)
  got, = _twice(lambda: _conv_residual(X, D, C, geom))
  ref = md.conv_residual64(x, d, c, case.stride, case.pad)
  err = md.rel(got, ref)
  gate = md.CONTRACTION_GATES['conv_residual ' + case.route[0]]
  _report(case.name, ' '.join(str(r) for r in case.route), err=err, gate=gate,
          masked=float((ref == 0).mean()))
  # the mask is exact: zero where the reference is zero (the data is dense)
  assert np.array_equal(got == 0, ref == 0)
  assert err < gate


# ----------------------------------------------------------- compute_metrics
SHORT_KEYS = {'Average LASSO L2 component': 'l2',
              'Average LASSO lagrange component': 'lagrange',
              'Average LASSO Loss': 'loss', 'Average Normalized L0': 'l0',
              'Average pSNR of reconstructions': 'psnr',
              'Average change in dictionary kernels': 'change'}


@pytest.mark.parametrize('mode', md.METRIC_MODES)
def test_compute_metrics_against_float64(device, mode):
  """Every key of TrainingStep.compute_metrics on given images and codes
  against sc_oracle.compute_metrics on float64 tensors, at shapes past one
  stride of every reduction, with one row reconstructed exactly."""
  from training import sparse_coding
  params = md.metrics_params(mode)
  x, c, d, previous = md.metrics_problem(mode)
  want = md.oracle_metrics(mode, x, c, d, previous, md.SPARSITY_WEIGHT,
                           params)
  X, C, D, P = (_dev(a, device) for a in (x, c, d, previous))
  step = sparse_coding.TrainingStep(D, params)
  step.sparsity_weight = md.SPARSITY_WEIGHT
  step.previous_dictionary = P
  runs = [step.compute_metrics(X, C) for _ in range(2)]
  for key in md.METRIC_KEYS:
    assert np.array_equal(np.asarray(runs[0][key]), np.asarray(runs[1][key]))
  errs = md.metric_errors(runs[0], want)
  _report('compute_metrics ' + mode, 'x'.join(str(v) for v in c.shape),
          **dict((SHORT_KEYS[key], err) for key, err in errs.items()))
  assert np.isfinite(float(want['Average pSNR of reconstructions']))
  for key, err in errs.items():
    assert err < md.METRIC_GATES[key], key
