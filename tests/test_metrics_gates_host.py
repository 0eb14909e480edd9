"""What the gates of tests/test_metrics_routes_gpu.py rest on, on the CPU.

The float64 restatements of tests/metrics_data.py, composed as
TrainingStep.compute_metrics composes the entry points, equal
sc_oracle.compute_metrics on the three runs of tests/golden/metrics.npz; every
case meets its input conditions and names the route the mirrors give on 256
compute units (and on 64, where that differs); and a numpy emulation of each
edge bug -- a dropped last element, element 256, last group, last K quarter
or last chunk of kernels, a counted -0.0, a flushed subnormal, the frame read
into the min / max -- misses the gate of every case it applies to."""
import numpy as np
import pytest
import torch

import helpers
import metrics_data as md
import sc_oracle


# ------------------------------------------------- restatements = the oracle
def _golden_run(tag):
  """(mode, params, validation batch, codes, dictionary, previous, lam) of a
  run of metrics.npz, the codes from the oracle's own inference."""
  g = helpers.load('metrics')
  params, _, val, d0, batch = helpers.metrics_cases(g)[tag]
  schedule = params['inference_param_schedule'][0]
  lam, iters = schedule['sparsity_weight'], schedule['num_iters']
  x = torch.from_numpy(val[:batch].copy())
  d = torch.from_numpy(d0.copy())
  if tag == 'conv':
    codes = sc_oracle.conv_ista_fista(x, d, params['strides'],
                                      params['padding'], lam, iters,
                                      variant='ista')
  elif tag == 'sub':
    codes = sc_oracle.subspace_ista_fista(x, d, params['group_assignments'],
                                          lam, iters)
  else:
    codes = sc_oracle.fc_ista_fista(x, d, lam, iters)
  rs = np.random.RandomState(5)
  previous = (d0 + 1e-3 * rs.randn(*d0.shape)).astype(np.float32)
  return tag, params, x.numpy(), codes.numpy(), d0, previous, lam


@pytest.mark.parametrize('tag', ['fc', 'sub', 'conv'])
def test_restatements_equal_the_oracle_on_the_golden_runs(tag):
  mode, params, x, c, d, previous, lam = _golden_run(tag)
  assert (c != 0).any()
  want = md.oracle_metrics(mode, x, c, d, previous, lam, params)
  got = md.metrics64(mode, x, c, d, previous, lam, params)
  for key, err in md.metric_errors(got, want).items():
    assert err < 1e-12, (key, err)


@pytest.mark.parametrize('mode', md.METRIC_MODES)
def test_restatements_equal_the_oracle_on_the_route_problems(mode):
  """The problems of test_compute_metrics_against_float64: past one stride,
  one row exact (left out of the pSNR mean), the frame outside the range."""
  params = md.metrics_params(mode)
  x, c, d, previous = md.metrics_problem(mode)
  want = md.oracle_metrics(mode, x, c, d, previous, md.SPARSITY_WEIGHT,
                           params)
  got = md.metrics64(mode, x, c, d, previous, md.SPARSITY_WEIGHT, params)
  for key, err in md.metric_errors(got, want).items():
    assert err < 1e-12, (key, err)
  b = x.shape[0]
  if mode == 'conv':
    residual = md.conv_residual64(x, d, c, params['strides'],
                                  params['padding'])
    assert c.shape[1:] == (20, 39, 46) and x.shape[1:] == (3, 45, 52)
    assert np.abs(x).max() == 9 and md.window_minmax64(md.Window(
        x.reshape(-1), 6 * 52 + 4, b * 3, 34, 42, 45 * 52, 52, None))[1] < 9
  else:
    residual = md.fc_residual64(x, d, c)
    assert x.shape == (37, 300) and c.shape == (37, 1030)
  if mode == 'sub':
    groups = params['group_assignments']
    assert len(groups) == 206 and len(set(len(g) for g in groups)) > 1
    assert sorted(a for g in groups for a in g) == list(range(1030))
  energy = (residual.reshape(b, -1) ** 2).sum(axis=1)
  assert energy[md.EXACT_ROW] == 0 and (np.delete(energy, md.EXACT_ROW)
                                        > 0).all()
  assert np.isfinite(want['Average pSNR of reconstructions'])


# ------------------------------------------------------------ route mirrors
def test_route_mirrors_agree_with_the_tables():
  for case in md.FC_RESIDUAL_CASES:
    assert md.gemm_route(case.b, case.n, md.CUS) == case.route, case.name
    assert md.gemm_route(case.b, case.n, md.CUS_SMALLER) == (
        case.route_smaller), case.name
  for case in md.GRAM_CASES:
    side, _ = md.gram_shape(case)
    assert md.gemm_route(side, side, md.CUS) == case.route, case.name
    assert md.gemm_route(side, side, md.CUS_SMALLER) == case.route_smaller, (
        case.name)
  for cases in (md.FC_RESIDUAL_CASES, md.GRAM_CASES):
    assert set(c.route for c in cases) == set(['gemm-small', 'gemm-big'])
    assert any(c.route != c.route_smaller for c in cases)
  for case in md.CONV_CASES:
    assert md.conv_route(case.kh, case.kw, case.stride, case.s) == (
        case.route), case.name
  assert set(c.route[0] for c in md.CONV_CASES) == set(['unit', 'plan'])
  # more than one chunk of kernels, the last one ragged
  assert any(c.route[0] == 'plan' and c.s > c.route[1] and
             c.route[2] != c.route[1] for c in md.CONV_CASES)
  for case in md.WINDOW_CASES:
    w = md.window_input(case)
    total = w.outer * w.rows * w.cols
    assert md.minmax_blocks(total) == case.blocks, case.name
  # the cap, and with it the grid-stride loop
  assert any(w.outer * w.rows * w.cols > md.MINMAX_BLOCKS * md.STAT_THREADS
             for w in map(md.window_input, md.WINDOW_CASES))


def test_k_quarter_edges_are_covered():
  """K of the small-kernel cases: below one quarter, one step past it, one
  below and one past the four quarters of 16, past several steps."""
  ks = set(c.s for c in md.FC_RESIDUAL_CASES if c.route == 'gemm-small')
  assert set([1, 15, 17, 63, 65, 1030]) <= ks
  ns = set(c.n for c in md.FC_RESIDUAL_CASES if c.route == 'gemm-small')
  assert set([1, 31, 33, 300]) <= ns
  assert set(c.b for c in md.FC_RESIDUAL_CASES) >= set([1, 37])
  assert md.small_k_quarter(63) == 16 and md.small_k_quarter(65) == 32
  assert md.small_k_quarter(1030) == 272


# --------------------------------------------------------- input conditions
@pytest.mark.parametrize('case', md.ROW_STATS_CASES,
                         ids=[c.name for c in md.ROW_STATS_CASES])
def test_row_stats_inputs_and_gate(case):
  x = md.row_stats_input(case)
  gate = md.reduction_gate(case.cols)
  assert np.isfinite(x).all() and x.shape == (case.rows, case.cols)
  assert md.edge_shares(x) >= md.EDGE_SHARE * gate
  sumsq, l1, l0 = md.row_stats64(x)
  tiny = (x != 0) & (np.abs(x) < 2.0 ** -126)
  minus_zero = (x == 0) & np.signbit(x)
  if case.kind == 'signed zeros':
    assert tiny.any(axis=1).all() and minus_zero.any(axis=1).all()
    # torch.norm(p=0), the reference's count
    assert np.array_equal(l0, torch.norm(torch.from_numpy(x.copy()).double(),
                                         p=0, dim=1).numpy())
  else:
    assert not tiny.any() and not minus_zero.any()
  faults = ['drop last element']
  if case.cols > md.STAT_THREADS:
    faults.append('drop element 256')
  for fault in faults:
    bad_sq, bad_l1, bad_l0 = md.row_stats64(x, fault)
    assert (np.abs(bad_sq - sumsq) > gate * sumsq).all(), fault
    assert (np.abs(bad_l1 - l1) > gate * l1).all(), fault
    assert (bad_l0 != l0).all(), fault
  if case.kind == 'signed zeros':
    for fault in ('count -0.0', 'flush subnormals'):
      assert (md.row_stats64(x, fault)[2] != l0).all(), fault


def test_reduction_gate_formula():
  """One stride: 11 roundings; 70 001 columns: 274 in the chain."""
  assert md.reduction_gate(256) == 1.01 * 11 * 2.0 ** -24
  assert md.reduction_gate(257) == 1.01 * 12 * 2.0 ** -24
  assert md.reduction_gate(70001) == 1.01 * 284 * 2.0 ** -24
  assert md.group_gate(700, 3) == 1.01 * (4 + 3 + 10) * 2.0 ** -24
  assert md.diff_gate(768) == 1.01 * (1 + 3 + 10 + 1) * 2.0 ** -24
  assert md.reduction_gate(70001) < 2e-5


@pytest.mark.parametrize('case', md.GROUP_CASES,
                         ids=[c.name for c in md.GROUP_CASES])
def test_group_inputs_and_gate(case):
  from vtc_hip import groups as group_tables
  codes, groups = md.group_input(case), md.group_lists(case)
  tables = group_tables.tables_for(groups, case.s, 'cpu')
  gate = md.group_gate(len(groups), tables.m)
  assert md.group_shares(codes, groups) >= md.EDGE_SHARE * gate
  ref = md.group_norm_sum64(codes, groups)
  assert ref[1] == 0 and (np.delete(ref, 1) > 0).all()
  bad = md.group_norm_sum64(codes, groups, 'drop last group')
  live = ref > 0
  assert (np.abs(bad - ref)[live] > gate * ref[live]).all()
  # the padded tables say what the lists say
  index = tables.index.numpy().reshape(len(groups), tables.m)
  valid = tables.valid.numpy().reshape(len(groups), tables.m).astype(bool)
  assert [list(index[g][valid[g]]) for g in range(len(groups))] == groups
  sizes = set(len(g) for g in groups)
  if case.kind == 'singletons':
    assert sizes == set([1])
    assert np.array_equal(ref, md.row_stats64(codes)[1])
  if case.kind in ('ragged', 'overlap'):
    assert sizes == set([1, 2, 3, 4, 5]) and not valid.all()
  if case.kind == 'overlap':
    flat = [a for g in groups for a in g]
    assert len(set(flat)) < len(flat)
  if case.kind == 'many':
    assert len(groups) == 700 > 2 * md.STAT_THREADS


@pytest.mark.parametrize('case', md.WINDOW_CASES,
                         ids=[c.name for c in md.WINDOW_CASES])
def test_window_inputs_and_gate(case):
  w = md.window_input(case)
  lo, hi = md.window_minmax64(w)
  assert (lo, hi) == (float(w.crop.min()), float(w.crop.max()))
  first, last = float(w.crop.reshape(-1)[0]), float(w.crop.reshape(-1)[-1])
  if case.kind == 'max first, min last':
    assert (first, last) == (hi, lo) and hi > lo
  if case.kind == 'min first, max last':
    assert (first, last) == (lo, hi) and hi > lo
  if case.kind == 'negative':
    assert hi < 0
  if case.kind == 'equal':
    assert lo == hi
  if case.pad is not None:
    assert w.offset > 0 and w.row_pitch > w.cols
    assert w.outer_pitch > w.rows * w.row_pitch
    bad = md.window_minmax64(w, 'read the frame')
    assert bad[0] == -1000 < lo and bad[1] == 1000 > hi


@pytest.mark.parametrize('case', md.DIFF_CASES,
                         ids=[c.name for c in md.DIFF_CASES])
def test_diff_inputs_and_gate(case):
  a, b = md.diff_input(case)
  gate = md.diff_gate(case.cols)
  assert md.diff_shares(a, b) >= md.EDGE_SHARE * gate
  ref = md.rows_mean_abs_diff64(a, b)
  live = np.arange(case.rows) != md.IDENTICAL_ROW
  assert ref[md.IDENTICAL_ROW] == 0 and (ref[live] > 0).all()
  faults = ['drop last element']
  if case.cols > md.STAT_THREADS:
    faults.append('drop element 256')
  for fault in faults:
    bad = md.rows_mean_abs_diff64(a, b, fault)
    assert (np.abs(bad - ref)[live] > gate * ref[live]).all(), fault


@pytest.mark.parametrize('case', md.FC_RESIDUAL_CASES,
                         ids=[c.name for c in md.FC_RESIDUAL_CASES])
def test_fc_residual_inputs_and_gate(case):
  x, d, c = md.fc_residual_input(case)
  ref = md.fc_residual64(x, d, c)
  ratio = np.linalg.norm(ref) / np.linalg.norm(x)
  assert 0.3 < ratio < 30, ratio       # not fitted: R of the order of X
  assert (c == 0).mean() > 0.2 or case.s == 1
  if case.route == 'gemm-small':
    bad = md.fc_residual64(x, d, c, 'drop last K quarter')
    assert md.rel(bad, ref) > md.CONTRACTION_GATES['fc_residual gemm-small']


@pytest.mark.parametrize('case', md.GRAM_CASES,
                         ids=[c.name for c in md.GRAM_CASES])
def test_gram_inputs_and_gate(case):
  a = md.gram_input(case)
  ref = md.gram64(a, case.transpose_a)
  side, k = md.gram_shape(case)
  assert ref.shape == (side, side) and md.rel(ref, ref.T) < 1e-15
  want = np.einsum('ki,kj->ij' if case.transpose_a else 'ik,jk->ij',
                   a.astype(np.float64), a.astype(np.float64))
  assert md.rel(ref, want) < 1e-15
  if case.route == 'gemm-small':
    bad = md.gram64(a, case.transpose_a, 'drop last K quarter')
    assert md.rel(bad, ref) > md.CONTRACTION_GATES['gram gemm-small']


@pytest.mark.parametrize('case', md.CONV_CASES,
                         ids=[c.name for c in md.CONV_CASES])
def test_conv_inputs_and_gate(case):
  x, d, c = md.conv_input(case)
  height, width = md.conv_image_shape(case)
  assert x.shape == (case.b, case.c, height, width)
  assert sc_oracle.conv_code_dim(height, case.kh, case.stride[0]) == case.ch
  assert sc_oracle.conv_code_dim(width, case.kw, case.stride[1]) == case.cw
  if case.route[0] == 'unit':
    assert height % 32 and width % 32
  ref = md.conv_residual64(x, d, c, case.stride, case.pad)
  mask = sc_oracle.conv_mask(torch.from_numpy(x), case.pad).numpy()
  assert np.array_equal(ref != 0, mask != 0)
  if case.pad is not None and 0 in (case.pad[0][1], case.pad[1][1]):
    assert not mask.any()          # the trailing 0 blanks everything
    return
  assert mask.any() and (case.pad is None) == bool(mask.all())
  ratio = np.linalg.norm(ref) / np.linalg.norm(x * mask)
  assert 0.3 < ratio < 30, ratio
  if case.route[0] == 'plan':
    bad = md.conv_residual64(x, d, c, case.stride, case.pad,
                             'drop last kernel chunk', case.route[1])
    assert md.rel(bad, ref) > md.CONTRACTION_GATES['conv_residual plan']


def test_conv_masks_cover_every_kind():
  kinds = set()
  for case in md.CONV_CASES:
    if case.pad is None:
      kinds.add('none')
    elif 0 in (case.pad[0][1], case.pad[1][1]):
      kinds.add('trailing 0')
    elif case.pad[0][0] == case.pad[0][1] and case.pad[1][0] == case.pad[1][1]:
      kinds.add('symmetric')
    else:
      kinds.add('asymmetric')
  assert kinds == set(['none', 'trailing 0', 'symmetric', 'asymmetric'])
  assert set(c.c for c in md.CONV_CASES if c.route[0] == 'unit') == set([1, 3])


def test_measured_gates_stay_in_the_f32_class():
  """Exact-f32 contractions: no measured gate above 1e-6."""
  for gates in (md.CONTRACTION_GATES, md.METRIC_GATES):
    assert all(0 < gate <= 1e-6 for gate in gates.values())
  assert sorted(md.METRIC_GATES) == md.METRIC_KEYS
