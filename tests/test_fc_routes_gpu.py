"""Every route of vtc_fc_ista_fista (csrc/fc_inference.hip) against float64.

One table of cases (tests/fc_routes_data.py) names, per case, the route it must
take -- fc_small, fc_chip16, the fused kernel (operand split, MFMA tile), the
streamed kernel, or the tiled loop (operand split, one-pass or split-K
residual, 16-byte or element-wise proximal epilogue); fc_route, a Python mirror
of the C dispatch, asserts it with the device's CU count, so a dispatch change
fails here instead of quietly moving coverage.  Per case: the plugin against
sc_oracle.fc_ista_fista on float64 inputs at the same explicit step size
(batches above 512 rows: a seeded sample of 256 rows, rows are independent),
and two runs bit for bit.  The options test runs ISTA, a warm start, the three
other thresholds, early stopping, the device-resident step size and the fused
kernel's other MFMA tile on the rows the table names.  The gates are the
project's own (helpers.REL_TOL_SHORT / NEAR_THRESHOLD; 1e-5 / 5e-6 on the bf16
hi/lo split); the single-part bf16 mode meets a float64 restatement with its
operands rounded to bf16, at four times that restatement's own sensitivity to
the summation order.  Hard thresholds leave out the rows in which a
pre-threshold value lies next to the cutoff.  tests/test_fc_gates_host.py shows
what the gates catch and that every case meets its input conditions.  Measured
errors: profiles/fc_routes.txt."""
import time

import pytest
import torch

import fc_routes_data as frd
import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fc():
  from analysis_transforms.fully_connected import ista_fista
  if not ista_fista.fused_available():
    pytest.fail('libvtc_hip.so was built without the fused FISTA kernel')
  start = time.perf_counter()
  yield ista_fista
  print('tests/test_fc_routes_gpu.py: %.1f s' % (time.perf_counter() - start))


def _cus():
  return torch.cuda.get_device_properties(0).multi_processor_count


def _report(name, route, what, err, flips, extra=''):
  print('%-40s %-44s %-5s rel %.2e  flips %d%s' % (
      name, '/'.join(str(r) for r in route), what, err, flips, extra))


def _problem(device, fc, case, option='fista'):
  """The case's problem on the device and its reference, the route asserted
  with this device's CU count."""
  import vtc_hip
  cus = _cus()
  p = frd.problem(case.name, cus)
  ref = frd.reference(case.name, cus, option)
  plain = frd.fc_route(p.b, case.n, case.s, case.precision, case.eps, frd.T,
                       cus)
  assert plain == case.route, case.name
  if 'tile' not in option.split():
    assert ref.route == case.route, (case.name, option)
  if ref.route[2:3] == ('split-k',):
    assert frd.x3_want_slices(p.b, case.n, case.s) > 1
  if ref.route[1:] == ('f32', 'single', 'wide'):
    assert not frd.gemm_prefers_small(p.b, case.s, cus)
  assert fc._resolve_precision('auto', p.b, case.n, case.s, None) == (
      vtc_hip.PRECISIONS[frd.auto_precision(case, cus)])
  return (p, ref, helpers.to_dev(p.X, device), helpers.to_dev(p.D, device),
          torch.from_numpy(ref.rows).to(device))


def _keywords(case, spec):
  nonneg, hard = frd.THRESHOLDS[spec.threshold]
  kw = dict(variant=spec.variant, precision=case.precision,
            nonnegative_only=nonneg, hard_threshold=hard)
  eps = case.stop_eps if spec.stop else case.eps
  if eps is not None:
    kw['early_stopping_epsilon'] = eps
  return kw


def _check(p, ref, route, ours, what, started):
  """Input conditions on the reference, then the gate on the rows kept."""
  name = '%s (%s)' % (p.case.name, what)
  frac, _, left_out = frd.assert_input_conditions(ref, name)
  tol, flip = ref.gate if route == ref.route else frd.gate(route)
  ours, want = ours[ref.keep], ref.ref64[ref.keep]
  err, flips = helpers.rel_err(ours, want), helpers.support_mismatch(
      ours, want)
  extra = '  active %.2f' % frac
  if 'hard' in ref.spec.threshold:
    extra += '  left out %d of %d' % ((~ref.keep).sum(), len(ref.keep))
  if ref.distance is not None:
    extra += '  bf16 distance %.2e gate %.2e' % (ref.distance, tol)
  _report(p.case.name, route, what, err, flips,
          extra + '  %.2f s' % (time.perf_counter() - started))
  helpers.assert_codes_match(ours, want, tol, name, max_flip_mag=flip)


@pytest.mark.parametrize('case', frd.CASES, ids=[c.name for c in frd.CASES])
def test_route_against_float64(device, fc, case):
  """FISTA, the soft threshold, T = 12, on every row of the case table."""
  started = time.perf_counter()
  p, ref, X, D, rows = _problem(device, fc, case)
  kw = _keywords(case, ref.spec)
  runs = [fc.run(X, D, case.lam, frd.T, stepsize=p.eta, **kw)
          for _ in range(2)]
  assert torch.equal(runs[0], runs[1]), case.name + ': runs differ'
  assert fc.run.last_iters == frd.T
  _check(p, ref, ref.route, runs[0][rows].cpu().numpy(), 'fista', started)
  if ref.route[0] == 'stream':
    # early stopping that never fires keeps the split and leaves the streamed
    # kernel: the tiled route computes the same codes in another order
    tiled = fc.run(X, D, case.lam, frd.T, stepsize=p.eta,
                   early_stopping_epsilon=0.0, **kw)
    assert fc.run.last_iters == frd.T
    assert not torch.equal(tiled, runs[0])
    route = frd.fc_route(p.b, case.n, case.s, case.precision, 0.0, frd.T,
                         _cus())
    assert route[:2] == ('tiled', ref.route[1])
    _check(p, ref, route, tiled[rows].cpu().numpy(), 'tiled', started)


@pytest.mark.parametrize('case,option', frd.OPTIONS,
                         ids=['%s-%s' % (c.name, o) for c, o in frd.OPTIONS])
def test_route_options(device, fc, monkeypatch, case, option):
  """ISTA, a warm start, the other thresholds, early stopping, the step size
  on the device, the fused kernel's other tile: where the table names them."""
  import vtc_hip
  started = time.perf_counter()
  spec = frd.option_spec(case, option)
  if spec.dev:
    p, ref, X, D, rows = _problem(device, fc, case)
    assert case.eps is None and vtc_hip.device_stepsize_available(case.n)
    kw = _keywords(case, ref.spec)
    on_device = fc.run(X, D, case.lam, frd.T, **kw)
    own = vtc_hip.stepsize_from_gram(vtc_hip.gram(D, True), D)
    by_value = fc.run(X, D, case.lam, frd.T, stepsize=own, **kw)
    assert torch.equal(on_device, by_value), case.name
    assert bool(on_device.any())
    vtc_hip.poll_spectrum_checks(block=True)
    print('%-40s %-44s %-5s bit for bit  %.2f s' % (
        case.name, '/'.join(str(r) for r in ref.route), option,
        time.perf_counter() - started))
    return
  p, ref, X, D, rows = _problem(device, fc, case, option)
  kw = _keywords(case, spec)
  if spec.tile:
    assert ref.route[2] != case.route[2]
    monkeypatch.setenv('VTC_FUSED_TILE', str(ref.route[2]))
  if spec.warm:
    init = helpers.to_dev(ref.init, device)
    keep = init.clone()
    kw['initial_codes'] = init
  runs = []
  for _ in range(2):
    runs.append(fc.run(X, D, case.lam, spec.iters, stepsize=p.eta, **kw))
    assert fc.run.last_iters == (ref.count if spec.stop else spec.iters), (
        fc.run.last_iters, ref.count)
  assert torch.equal(runs[0], runs[1]), case.name + ': runs differ'
  if spec.warm:
    assert torch.equal(init, keep)
  if spec.stop:
    print('%-40s stopped after %d iterations, float64 oracle %d' % (
        case.name, fc.run.last_iters, ref.count))
  _check(p, ref, ref.route, runs[0][rows].cpu().numpy(), option, started)


def test_refusals(device, fc):
  """bf16 outside the fused kernel and a split mode at n or s that is no
  multiple of 4 raise; 'auto' runs the exact-f32 kernels there."""
  cus = _cus()
  for precision, b, n, s in frd.REFUSALS:
    assert frd.fc_route(b, n, s, precision, None, 5, cus)[0] == 'refused'
    X = helpers.to_dev(helpers.gaussian_patches(1, b, n), device)
    D = helpers.to_dev(helpers.unit_rows(2, s, n), device)
    with pytest.raises(NotImplementedError):
      fc.run(X, D, 0.05, 5, precision=precision, stepsize=0.3)
    auto = fc.run(X, D, 0.05, 5, precision='auto', stepsize=0.3)
    f32 = fc.run(X, D, 0.05, 5, precision='f32', stepsize=0.3)
    assert torch.equal(auto, f32) and bool(f32.any())
