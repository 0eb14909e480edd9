"""CPU checks behind tests/test_subspace_routes_gpu.py: the dispatch mirror
gives every case of the table its named route at 256 CUs, the float64
iteration in grouped form (subspace_routes_data.grouped_iterates) agrees with
sc_oracle, and the gates of the route tests notice what these kernels can get
wrong -- each mutation below, applied to the float64 codes of a case at the
rows the GPU test compares, fails helpers.assert_codes_match at the case's
gate.  No GPU needed."""
import numpy as np
import pytest
import torch

import helpers
import subspace_routes_data as srd

CUS = 256      # MI355X

GATED = ['1 f32 epilogue m=8', '1 f32 epilogue m=32',
         '4 f32 group kernel stride loop m=3', '9 f32 ragged overlapping']


@pytest.mark.parametrize('case', srd.CASES, ids=[c.name for c in srd.CASES])
def test_dispatch_mirror_names_each_case(case):
  b = srd.batch_size(case, CUS)
  slots = case.groups * case.m
  for eps in (None,) if case.stop_eps is None else (None, case.stop_eps):
    assert srd.subspace_route(b, case.n, case.groups, case.m, case.precision,
                              eps, CUS) == case.route
  groups, atoms = srd.group_lists(case)
  assert len(groups) == case.groups and max(map(len, groups)) == case.m
  assert sorted(set(a for g in groups for a in g)) == list(range(atoms))
  family, split, residual, prox = case.route
  # the sizes that put the case on its branch (csrc/subspace.hip)
  if case.name.startswith('1 ') or case.name.startswith('9 f32'):
    assert not srd.gemm_prefers_small(b, slots, CUS)
    assert srd.gemm_prefers_small(b - 106, slots, CUS)
    assert b % 128 and b % 32 and slots % 128 and slots % 32 == 0
  if case.name.startswith('3 '):
    assert b * slots // 4 > 8192 * 256          # rounds > 1
  if case.name.startswith('4 '):
    assert b * case.groups > 4096 * 256          # the stride loop
    assert srd.gemm_prefers_small(b, slots, CUS)
  if case.name.startswith('5 '):
    assert b * case.groups > 4096 * 256
    assert not srd.gemm_prefers_small(b, slots, CUS)
  if case.name.startswith('6 '):
    assert case.m in (1, 2) and b * slots % 4
  if case.name.startswith('7 '):
    assert b > 256 and b % 128
  if residual == 'split-k':
    assert srd.x3_want_slices(b, case.n, slots) > 1
  if case.name.startswith('9 '):
    assert any(len(g) < case.m for g in groups)
    shared = [a for g in groups for a in g]
    assert len(shared) > atoms                  # atoms in two groups
    # gather_cols_kernel / scatter_add_kernel past their 4096 * 256 threads
    assert case.precision != 'f32' or b * atoms > 4096 * 256


def test_dispatch_mirror_boundaries():
  route = srd.subspace_route
  # f16x3 falls to the bf16 split where the epilogue has no group shape
  assert route(40, 64, 20, 12, 'f16x3', None, CUS)[1:] == (
      'bf16', 'single', 'group-kernel')
  assert route(40, 64, 5, 64, 'f16x3', None, CUS)[1:] == (
      'bf16', 'split-k', 'pow2-kernel')
  # the streamed kernel: n = 256, whole 256-slot phases, m <= 8, no stopping
  assert route(45, 256, 96, 8, 'bf16x3', None, CUS)[0] == 'stream'
  assert route(45, 256, 96, 8, 'bf16x3', 1e-3, CUS)[0] == 'tiled'
  assert route(45, 256, 96, 8, 'f32', None, CUS)[0] == 'tiled'
  assert route(45, 256, 48, 16, 'f16x3', None, CUS)[0] == 'tiled'
  assert route(45, 256, 100, 8, 'f16x3', None, CUS)[0] == 'tiled'
  assert route(45, 128, 96, 8, 'f16x3', None, CUS)[0] == 'tiled'
  assert route(45, 256, 4096, 8, 'f16x3', None, CUS)[0] == 'tiled'
  # the real subspace configuration under precision='f32'
  assert route(8192, 256, 512, 8, 'f32', None, CUS) == srd.E32
  assert route(512, 256, 512, 8, 'f32', None, CUS) == srd.P32
  # f32, slots not a multiple of 4: no epilogue, the shuffle kernel while
  # b * slots is one
  assert route(40000, 24, 1057, 1, 'f32', None, CUS) == srd.P32
  assert route(40001, 24, 1057, 1, 'f32', None, CUS) == srd.G32


@pytest.mark.parametrize('name', GATED + ['10 stream ragged 8-5-3'])
@pytest.mark.parametrize('variant', ['fista', 'ista'])
def test_grouped_iteration_matches_oracle(name, variant):
  p = srd.problem(name, CUS)
  rows = p.rows[:32]
  codes, _, _ = srd.grouped_iterates(p, rows, srd.T, variant)
  ref = srd.oracle(p, torch.float64, srd.T, variant, rows).numpy()
  assert helpers.rel_err(srd.scatter(p, codes[-1]), ref) < 1e-13
  assert not codes[-1][:, p.valid == 0].any()


def _mutations(p):
  """name -> float64 (rows, atoms) codes after T iterations with one fault in
  the last iteration."""
  case, m = p.case, p.case.m
  rows = p.rows
  X = p.X[rows].astype(np.float64)
  codes, points, dg = srd.grouped_iterates(p, rows, srd.T)
  last, before, y = codes[-1], codes[-2], points[-1]
  rs = np.random.RandomState(11)
  out = {}

  def neighbour_norm(pre):
    norms = srd.group_norms(p, pre).copy().reshape(len(rows), -1, m)
    pick = rs.randint(0, case.groups - 1, len(rows))
    norms[np.arange(len(rows)), pick] = norms[np.arange(len(rows)), pick + 1]
    return norms.reshape(pre.shape)
  out['a neighbour norm'] = srd.group_step(p, X, dg, y, neighbour_norm)
  if m > 1:
    out['b norm misses last member'] = srd.group_step(
        p, X, dg, y, lambda pre: srd.group_norms(p, pre, m - 1))
  # c: one row of the sample (0.03 % of the rows, rounded up), one piece
  stale = last.copy()
  row = rs.randint(len(rows))
  pieces = np.nonzero(last[row, ::4] != before[row, ::4])[0]
  col = 4 * pieces[rs.randint(len(pieces))]
  stale[row, col] = before[row, col]
  out['c stale first element of a piece'] = stale
  tail = last.copy()
  tail[:, -4:] = 0
  out['d last 4 columns zero'] = tail
  edge = p.rows >= 128 * (p.b // 128)
  assert 0 < edge.sum() < len(rows)
  behind = last.copy()
  behind[edge] = before[edge]
  out['e ragged row tile one iteration behind'] = behind
  out = dict((k, srd.scatter(p, v)) for k, v in out.items())
  if not p.valid.all():
    # f: a padded slot holds its group's first code and the scatter takes it
    # (slot -> atom 0, the index table's filler)
    live = last.copy().reshape(len(rows), case.groups, m)
    pad = (p.valid == 0).reshape(case.groups, m)
    live[:, pad] = np.broadcast_to(live[:, :, :1], live.shape)[:, pad]
    out['f padded slots live'] = srd.scatter(
        p, live.reshape(last.shape), masked=False)
  return out


@pytest.mark.parametrize('name', GATED)
def test_gates_catch_kernel_faults(name):
  p = srd.problem(name, CUS)
  tol, flip = srd.gate(p.case.route)
  ref64, ref32 = srd.reference(name, CUS)
  srd.assert_input_conditions(p, ref64, ref32, name)
  # the float32 copy itself passes
  helpers.assert_codes_match(ref64.astype(np.float32), ref64, tol, name,
                             max_flip_mag=flip)
  faults = _mutations(p)
  assert len(faults) == (6 if not p.valid.all() else 5)
  missed = []
  for fault, codes in sorted(faults.items()):
    bad = codes.astype(np.float32)
    flips = (bad != 0) != (ref64 != 0)
    worst = np.maximum(np.abs(bad), np.abs(ref64))[flips].max() if (
        flips.any()) else 0.0
    print('%-36s %-40s rel %.2e (gate %.0e)  largest flip %.1e' % (
        name, fault, helpers.rel_err(bad, ref64), tol, worst))
    try:
      helpers.assert_codes_match(bad, ref64, tol, fault, max_flip_mag=flip)
      missed.append(fault)
    except AssertionError:
      pass
  assert not missed, missed
