"""Every route of vtc_conv_ista_fista (csrc/conv.hip) against float64.

One table of cases (tests/conv_routes_data.py) names, per case, the route it
must take: the kernel family (fused or two-kernel split contractions, patch
contractions, stride-1 scalar-tap kernels, direct kernels, or the unit
synthesis with the direct analysis) and, inside it, what cx_fill_plan,
unit_groups and plan_analysis chose.  conv_route, a Python mirror of the C
dispatch, asserts it with the device's CU count, so a dispatch change fails
here instead of quietly moving coverage.  Per case: FISTA, T = 12, at the
convergent step 1 / (cover * lambda_max(F F^T)) against
sc_oracle.conv_ista_fista on float64 inputs (large batches: a few sampled
images, images are independent), and two runs bit for bit.  The gates are the
project's own (helpers.REL_TOL_SHORT / NEAR_THRESHOLD; 2e-5 / 1e-5 on the bf16
split); tests/test_conv_gates_host.py shows what they catch.  Each test
asserts on its references that the case is not degenerate: 10-90 % of the
codes non-zero, none above 10, the float32 oracle within half the gate with no
support flip above NEAR_THRESHOLD.  Cases whose mask has a trailing pad of 0
keep exactly zero codes.  Measured errors: profiles/conv_routes.txt."""
import ctypes

import numpy as np
import pytest
import torch

import conv_routes_data as crd
import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def conv():
  from analysis_transforms.convolutional import ista_fista
  return ista_fista


def _cus():
  return torch.cuda.get_device_properties(0).multi_processor_count


def _report(name, route, what, err, flips, frac):
  print('%-40s %-44s %-7s rel %.2e  flips %d  active %.2f' % (
      name, '/'.join(str(r).replace(' ', '') for r in route), what, err, flips,
      frac))


def _problem(device, case):
  """The case's problem on the device, its geometry and route asserted.
  Returns (problem, route, images, kernels, sampled image indices, whether
  vtc_conv_x3_supported accepts the geometry)."""
  import vtc_hip
  from utils import convolutions
  p = crd.problem(case.name)
  X, D = helpers.to_dev(p.X, device), helpers.to_dev(p.D, device)
  geom = convolutions.geometry(X, D, case.stride, p.pad)
  assert crd.same_geometry(p.geom, geom), case.name
  supported = bool(vtc_hip.load_library().vtc_conv_x3_supported(
      ctypes.byref(geom)))
  plan = crd.x3_plan(p.geom, _cus())
  # (the mirror leaves out cx_pick_rows: it may only accept more)
  assert not supported or (plan is not None and plan.supported), case.name
  assert supported or case.precision == 'f32', case.name
  route = crd.conv_route(p.geom, case.precision, _cus())
  assert route == case.route, case.name
  return p, route, X, D, torch.from_numpy(p.images).to(device), supported


def _check(p, gate, route, ours, ref64, ref32, what, stop=None):
  """Input conditions on the references, then the gate."""
  name = '%s (%s)' % (p.case.name, what)
  tol, flip = gate
  frac, _ = crd.assert_input_conditions(p, ref64, ref32, name, tol, stop)
  err = helpers.rel_err(ours, ref64) if ref64.any() else float(
      np.abs(ours).max())
  _report(p.case.name, route, what, err,
          helpers.support_mismatch(ours, ref64), frac)
  helpers.assert_codes_match(ours, ref64, tol, name, max_flip_mag=flip)


@pytest.mark.parametrize('case', crd.CASES, ids=[c.name for c in crd.CASES])
def test_route_against_float64(device, conv, case):
  """FISTA, T = 12, on every row of the case table."""
  from utils import convolutions
  p, route, X, D, images, supported = _problem(device, case)

  def run(precision):
    out = conv.run(X, D, case.stride, p.pad, case.lam, crd.T, stepsize=p.eta,
                   precision=precision)
    assert conv.run.last_iters == crd.T
    return out

  runs = [run(case.precision) for _ in range(2)]
  assert torch.equal(runs[0], runs[1]), case.name + ': runs differ'
  ref64, ref32 = crd.reference(case.name)
  _check(p, crd.gate(route), route, runs[0][images].cpu().numpy(), ref64,
         ref32, 'fista')
  if crd.blank_axis(case):
    # the whole batch, not only through the gate
    assert not bool(runs[0].any()), case.name + ': codes under a blank mask'
  # 'auto': the mirror of _resolve_precision first, then the same bits
  auto = crd.resolve_precision('auto', p.geom, False, supported)
  geom = convolutions.geometry(X, D, case.stride, p.pad)
  assert conv._resolve_precision('auto', geom, False) == auto
  assert conv._resolve_precision('auto', geom, True) == 'f32'
  if auto == case.precision:
    assert torch.equal(run('auto'), runs[0]), case.name + ": 'auto' differs"
  if case.precision != 'f32' and crd.twin(case.name) == case.name:
    # the same geometry through the exact-f32 kernels (the unit route)
    exact = run('f32')
    f32_route = crd.conv_route(p.geom, 'f32', _cus())
    assert f32_route[0] in ('unit', 'unit-synth+direct')
    _check(p, crd.GATE_F32, f32_route, exact[images].cpu().numpy(), ref64,
           ref32, 'f32')
    if crd.blank_axis(case):
      assert not bool(exact.any())


OPTIONS = [(c, o) for c in crd.OPTION_CASES for o in crd.OPTIONS]


@pytest.mark.parametrize('case,option', OPTIONS,
                         ids=['%s %s' % (c.name, o) for c, o in OPTIONS])
def test_route_options(device, conv, case, option):
  """ISTA, a warm start, early stopping and the threshold modes, on one
  representative per family and split mode."""
  p, route, X, D, images, _ = _problem(device, case)
  gate = crd.gate(route)
  lam, iters, count, eta = case.lam, crd.T, None, p.eta
  kw = dict(precision=case.precision)
  if option == 'ista':
    ref64, ref32 = crd.reference(case.name, 'ista')
    kw['variant'] = 'ista'
  elif option == 'warm':
    init, ref64, ref32 = crd.warm_reference(case.name)
    init = helpers.to_dev(init, device)
    keep = init.clone()
    iters = crd.WARM_ITERS
    kw['initial_codes'] = init
  elif option == 'stop':
    # a mean over the whole batch (no option case is sampled)
    assert case.sample is None
    ref64, ref32, count = crd.stop_reference(case.name)
    iters = crd.STOP_ITERS
    kw.update(variant='ista', early_stopping_epsilon=case.stop_eps)
  elif option == 'nonneg':
    ref64, ref32 = crd.reference(case.name, 'fista', True)
    kw['nonnegative_only'] = True
  else:
    # one iteration: a hard threshold is discontinuous, an entry within
    # rounding distance of the cutoff flips by the cutoff and moves its
    # neighbours from then on (tests/test_conv_gpu.py).  The cutoff and the
    # gate are that test's: flips only at lambda * eta = 1e-3, under codes
    # large enough that one flip fits the relative gate (crd.hard_step)
    ref64, ref32 = crd.hard_reference(case.name)
    lam, eta = crd.hard_lam(case.name), crd.hard_step(case.name)
    iters, gate = 1, crd.HARD_GATE
    kw['hard_threshold'] = True
  runs = []
  for _ in range(2):
    runs.append(conv.run(X, D, case.stride, p.pad, lam, iters, stepsize=eta,
                         **kw))
    if option == 'stop':
      print('%-40s stopped after %d iterations, float64 oracle %d' % (
          case.name, conv.run.last_iters, count))
      assert 1 < conv.run.last_iters < crd.STOP_ITERS
      assert conv.run.last_iters == count
    else:
      assert conv.run.last_iters == iters
  assert torch.equal(runs[0], runs[1]), case.name + ': runs differ'
  if option == 'warm':
    assert torch.equal(init, keep)
  ours = runs[0][images].cpu().numpy()
  if option == 'hard':
    frac = crd.active_fraction(ref64)
    assert 0.0 < frac < 1.0
    assert gate[1] / np.linalg.norm(ref64) <= gate[0] / 4
    helpers.assert_codes_match(ref32, ref64, gate[0] / 2, case.name + ' hard',
                               max_flip_mag=gate[1])
    _report(case.name, route, option, helpers.rel_err(ours, ref64),
            helpers.support_mismatch(ours, ref64), frac)
    helpers.assert_codes_match(ours, ref64, gate[0], case.name + ' hard',
                               max_flip_mag=gate[1])
  else:
    _check(p, gate, route, ours, ref64, ref32, option,
           (crd.stop_trace(case.name)[1], count) if option == 'stop' else None)
