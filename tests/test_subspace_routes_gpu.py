"""Every route of vtc_subspace_ista_fista (csrc/subspace.hip) against float64.

One table of cases (tests/subspace_routes_data.py) names, per case, the route
(kernel family, operand split, residual product, proximal step) it must take;
_subspace_route, a Python mirror of the C dispatch, asserts it, so a dispatch
change fails here instead of quietly moving coverage.  Per case: the plugin
against sc_oracle.subspace_ista_fista on float64 inputs at the same explicit
step size (batches above 512 rows: a seeded sample of 256 rows, rows are
independent), and two runs bit for bit.  The gates are the project's own
(helpers.REL_TOL_SHORT / NEAR_THRESHOLD; 2e-5 / 1e-5 on the bf16 split);
tests/test_subspace_gates_host.py shows what they catch.  Each test asserts on
its float64 reference that the case is not degenerate: 10-90 % of the groups
active, the float32 oracle within half the gate with no support flip above
NEAR_THRESHOLD.  Measured errors: profiles/subspace_routes.txt."""
import ctypes

import numpy as np
import pytest
import torch

import helpers
import subspace_routes_data as srd
from test_fused_stream_gpu import _routes_to_the_streamed_kernel

pytestmark = pytest.mark.gpu

_x3_want_slices = srd.x3_want_slices


@pytest.fixture(scope='module')
def sub():
  from analysis_transforms.fully_connected import subspace_ista_fista
  return subspace_ista_fista


def _cus():
  return torch.cuda.get_device_properties(0).multi_processor_count


def _gemm_prefers_small(m, n):
  """gemm_prefers_small (csrc/gemm_f32.h), as in test_update_routes_gpu.py."""
  return srd.gemm_prefers_small(m, n, _cus())


def _subspace_route(b, n, groups, m, precision, eps, cus):
  """(family, split, residual, prox) of vtc_subspace_ista_fista."""
  return srd.subspace_route(b, n, groups, m, precision, eps, cus)


def _report(name, route, what, err, flips, extra=''):
  print('%-40s %-44s %-5s rel %.2e  flips %d%s' % (
      name, '/'.join(str(r) for r in route), what, err, flips, extra))


def _problem(device, case, eps=None):
  """The case's problem on the device, its route asserted."""
  cus = _cus()
  p = srd.problem(case.name, cus)
  route = _subspace_route(p.b, case.n, case.groups, case.m, case.precision,
                          eps, cus)
  assert route == case.route, case.name
  if route[0] == 'stream':
    assert _routes_to_the_streamed_kernel(p.b, p.slots, case.m)
  if route[2] == 'split-k':
    assert _x3_want_slices(p.b, case.n, p.slots) > 1
  if route[3] == 'epilogue' and route[1] == 'f32':
    assert not _gemm_prefers_small(p.b, p.slots)
  return (p, route, helpers.to_dev(p.X, device), helpers.to_dev(p.D, device),
          torch.from_numpy(p.rows).to(device))


def _check(p, route, ours, ref64, ref32, what):
  """Input conditions on the reference, then the case's gate."""
  name = '%s (%s)' % (p.case.name, what)
  frac, _ = srd.assert_input_conditions(p, ref64, ref32, name)
  tol, flip = srd.gate(route)
  err, flips = helpers.rel_err(ours, ref64), helpers.support_mismatch(
      ours, ref64)
  _report(p.case.name, route, what, err, flips, '  active %.2f' % frac)
  helpers.assert_codes_match(ours, ref64, tol, name, max_flip_mag=flip)


def _grouped_codes(p, X, D):
  """The padded (b, slots) codes of vtc_subspace_ista_fista, as the plugin
  calls it, before vtc_group_scatter_add."""
  import vtc_hip
  from vtc_hip import groups as group_tables
  lib = vtc_hip.load_library()
  case, device = p.case, X.device
  stream = vtc_hip.current_stream(device)
  t = group_tables.tables_for(p.groups, p.atoms, device)
  assert (t.slots, t.num_groups, t.m) == (p.slots, case.groups, case.m)
  dg = torch.empty((p.slots, case.n), dtype=torch.float32, device=device)
  vtc_hip.check(lib.vtc_group_gather_rows(
      vtc_hip.ptr(D), vtc_hip.ptr(t.index), vtc_hip.ptr(t.valid),
      vtc_hip.ptr(dg), p.slots, case.n, stream), 'vtc_group_gather_rows')
  grouped = torch.full((p.b, p.slots), float('nan'), device=device)
  ws = vtc_hip.workspace(lib.vtc_subspace_ista_fista_workspace_bytes(
      p.b, case.n, case.groups, case.m), device)
  iters = ctypes.c_int(0)
  vtc_hip.check(lib.vtc_subspace_ista_fista(
      vtc_hip.ptr(X), vtc_hip.ptr(dg), vtc_hip.ptr(None), vtc_hip.ptr(grouped),
      p.b, case.n, case.groups, case.m, p.eta, case.lam, srd.T,
      vtc_hip.variant_code('fista'), -1.0, vtc_hip.PRECISIONS[case.precision],
      vtc_hip.ptr(ws), ws.numel(), ctypes.byref(iters), stream),
      'vtc_subspace_ista_fista')
  assert iters.value == srd.T
  return grouped, t


@pytest.mark.parametrize('case', srd.CASES, ids=[c.name for c in srd.CASES])
def test_route_against_float64(device, sub, case):
  """FISTA, T = 12, on every row of the case table."""
  p, route, X, D, rows = _problem(device, case)
  runs = [sub.run(X, D, p.groups, case.lam, srd.T, stepsize=p.eta,
                  precision=case.precision) for _ in range(2)]
  assert torch.equal(runs[0], runs[1]), case.name + ': runs differ'
  assert sub.run.last_iters == srd.T
  ref64, ref32 = srd.reference(case.name, _cus())
  _check(p, route, runs[0][rows].cpu().numpy(), ref64, ref32, 'fista')
  if route[0] == 'stream':
    # early stopping that never fires keeps the split and leaves the streamed
    # kernel: the tiled route computes the same codes in another order
    tiled = sub.run(X, D, p.groups, case.lam, srd.T, stepsize=p.eta,
                    precision=case.precision, early_stopping_epsilon=0.0)
    assert sub.run.last_iters == srd.T
    assert not torch.equal(tiled, runs[0])
    _check(p, _subspace_route(p.b, case.n, case.groups, case.m,
                              case.precision, 0.0, _cus()),
           tiled[rows].cpu().numpy(), ref64, ref32, 'tiled')
  if case.layout != 'contiguous':
    # padded slots hold zero dictionary rows: their codes stay exactly zero,
    # and the plugin's codes are the sums over each atom's slots
    grouped, t = _grouped_codes(p, X, D)
    pad = torch.from_numpy(p.valid == 0).to(device)
    assert int(pad.sum()) > 0
    assert bool((grouped[:, pad] == 0).all())
    summed = torch.zeros_like(runs[0])
    keep = torch.from_numpy(np.nonzero(p.valid)[0]).to(device)
    summed.index_add_(1, t.index[keep].long(), grouped[:, keep])
    # (an atom sits in at most two slots: the sum has one rounding order)
    assert torch.equal(summed, runs[0]), case.name + ': sum over slots'


OPTIONS = [(c, o) for c in srd.OPTION_CASES for o in ('ista', 'warm', 'stop')]
# gather_cols_kernel past its grid on ragged groups, shared atoms gathered twice
OPTIONS.append((srd.BY_NAME['9 f32 ragged overlapping'], 'warm'))


@pytest.mark.parametrize('case,option', OPTIONS,
                         ids=['%s %s' % (c.name, o) for c, o in OPTIONS])
def test_route_options(device, sub, case, option):
  """ISTA, a warm start and early stopping, once per proximal step."""
  cus = _cus()
  kw = dict(precision=case.precision)
  if option == 'ista':
    p, route, X, D, rows = _problem(device, case)
    ref64, ref32 = srd.reference(case.name, cus, 'ista')
    args = (srd.T,)
    kw['variant'] = 'ista'
  elif option == 'warm':
    p, route, X, D, rows = _problem(device, case)
    init, ref64, ref32 = srd.warm_reference(case.name, cus)
    init = helpers.to_dev(init, device)
    keep = init.clone()
    args = (srd.WARM_ITERS,)
    kw['initial_codes'] = init
  else:
    p, route, X, D, rows = _problem(device, case, case.stop_eps)
    ref64, ref32, count = srd.stop_reference(case.name, cus)
    rows = torch.arange(p.b, device=device)
    args = (srd.STOP_ITERS,)
    kw.update(variant='ista', early_stopping_epsilon=case.stop_eps)
  runs = []
  for _ in range(2):
    runs.append(sub.run(X, D, p.groups, case.lam, *args, stepsize=p.eta,
                        **kw))
    if option == 'stop':
      print('%-40s stopped after %d iterations, float64 oracle %d' % (
          case.name, sub.run.last_iters, count))
      assert 1 < sub.run.last_iters < srd.STOP_ITERS
      assert sub.run.last_iters == count
    else:
      assert sub.run.last_iters == args[0]
  assert torch.equal(runs[0], runs[1]), case.name + ': runs differ'
  if option == 'warm':
    assert torch.equal(init, keep)
  _check(p, route, runs[0][rows].cpu().numpy(), ref64, ref32, option)
