"""CPU checks behind tests/test_fc_routes_gpu.py: the dispatch mirror
(fc_routes_data.fc_route) gives every case of the table its named route at 256
and at 64 CUs and turns where fc_ista_fista_impl and run_generic turn, 'auto'
resolves as the table states, every case and option meets its input conditions
(active share, float32 oracle within half the gate, rows left out by a hard
threshold), the float64 iteration in numpy agrees with sc_oracle, and the gates
notice what these kernels can get wrong -- each fault of fc_routes_data.FAULTS,
applied to that iteration at the rows the GPU test compares, fails
helpers.assert_codes_match at the case's gate.  No GPU needed."""
import numpy as np
import pytest
import torch

import fc_routes_data as frd
import helpers

CUS = 256      # MI355X

GATED = ['2 fused f16x3 s=1024', '2 fused bf16 s=256',
         '4 f32 wide past the cut-over', '5 bf16x3 split-K']
# fault -> the option whose gate must notice it
FAULT_OPTION = {
    'momentum one ahead': 'fista',
    'cutoff lam': 'fista',
    'nonneg keeps negatives': 'fista soft_nonneg',
    'hard subtracts the cutoff': 'fista hard',
    'stale column tile': 'fista',
    'last rows from the row above': 'fista',
    'warm start misses the evaluation point': 'warm'}


@pytest.fixture
def resolve(monkeypatch):
  """_resolve_precision('auto', ...) of the plugin, without the library."""
  import vtc_hip
  from analysis_transforms.fully_connected import ista_fista
  monkeypatch.setattr(ista_fista, 'fused_available', lambda: True)
  names = dict((v, k) for k, v in vtc_hip.PRECISIONS.items())
  return lambda b, n, s, eps: names[
      ista_fista._resolve_precision('auto', b, n, s, eps)]


@pytest.mark.parametrize('case', frd.CASES, ids=[c.name for c in frd.CASES])
def test_dispatch_mirror_names_each_case(case, resolve):
  for cus in (256, 64):
    b = frd.batch_size(case, cus)
    assert frd.fc_route(b, case.n, case.s, case.precision, case.eps, frd.T,
                        cus) == case.route
    for option in case.options:
      route = frd.option_route(case, option, b, cus)
      if 'tile' in option:
        assert route == case.route[:2] + (48 - case.route[2],)
      else:
        assert route == case.route, option
    assert resolve(b, case.n, case.s, None) == frd.auto_precision(case, cus)
    if case.route[2:3] == ('split-k',):
      assert frd.x3_want_slices(b, case.n, case.s) > 1
    if case.route[2:3] == ('single',) and case.route[1] != 'f32':
      assert frd.x3_want_slices(b, case.n, case.s) == 1
    # the sizes that put the case on its branch (csrc/fc_inference.hip)
    if case.name == '4 f32 wide past the cut-over':
      assert not frd.gemm_prefers_small(b, case.s, cus)
      assert frd.gemm_prefers_small(b - 38, case.s, cus)
      assert b % 128           # a ragged last 128-row tile
    if case.name == '4 f32 element below the cut-over':
      assert frd.gemm_prefers_small(b, case.s, cus) and case.s % 4 == 0
      assert b > 512
    if case.name == '4 f32 element s=201 past the cut-over':
      # the element-wise epilogue behind the 128 x 128 kernel, not the 32 x 32
      assert not frd.gemm_prefers_small(b, case.s, cus) and case.s % 4
    if case.name == '4 f32 element s=201':
      assert frd.gemm_prefers_small(b, case.s, cus)
    if case.name == '4 f32 at a fused shape':
      assert frd.gemm_prefers_small(b, case.s, cus)
    if case.name.startswith('2 fused'):
      assert b > 64 and b % 32
  if case.stop_eps is not None:
    assert 'stop' in case.options and case.route[0] == 'tiled'
  assert frd.auto_precision(case, CUS) in ('f32', 'f16x3')


def test_auto_on_the_refused_shapes_and_under_early_stopping(resolve):
  for precision, b, n, s in frd.REFUSALS:
    assert frd.fc_route(b, n, s, precision, None, frd.T, CUS)[0] == 'refused'
    assert resolve(b, n, s, None) == 'f32'
    assert frd.fc_route(b, n, s, 'f32', None, frd.T, CUS)[0] in (
        'small', 'tiled')
  # an epsilon takes the fused and the on-chip shapes' own precision away
  assert resolve(96, 256, 256, 1e-3) == 'f32'
  assert resolve(96, 256, 256, None) == 'f16x3'


def test_dispatch_mirror_boundaries():
  route = lambda b, n, s, prec, eps=None, iters=frd.T, cus=CUS: frd.fc_route(
      b, n, s, prec, eps, iters, cus)
  # s = 192 / 256 at n = 64: small -> chip16
  assert route(33, 64, 192, 'f32') == ('small', 'f32')
  assert route(33, 64, 256, 'f32') == ('chip16', 'f32')
  assert route(33, 64, 320, 'f32')[0] == 'tiled'
  # s = 1024 / 1152 / 1280: fused -> tiled -> stream; 768 streams (six phases)
  for prec, split in (('f16x3', 'f16'), ('bf16x3', 'bf16x2')):
    assert route(45, 256, 1024, prec)[:2] == ('fused', split)
    assert route(45, 256, 1152, prec) == ('tiled', split, 'split-k', 'wide')
    assert route(45, 256, 1280, prec) == ('stream', split)
    assert route(45, 256, 768, prec) == ('stream', split)
    assert route(45, 256, 384, prec)[0] == 'tiled'
    assert route(45, 252, 768, prec)[0] == 'tiled'
    # s = 16384 / 16640
    assert route(8, 256, 16384, prec) == ('stream', split)
    assert route(8, 256, 16640, prec) == ('tiled', split, 'split-k', 'wide')
  assert route(45, 256, 1024, 'f16x3')[2] == 16
  assert route(45, 256, 1024, 'bf16')[2] == 16
  assert route(45, 256, 1024, 'bf16x3')[2] == 32
  assert route(45, 256, 768, 'bf16')[0] == 'refused'
  # T = 16384 / 16385: the momentum table of the on-chip kernels
  for n, s, prec, family in ((64, 128, 'f32', 'small'),
                             (144, 288, 'f32', 'chip16'),
                             (256, 512, 'f16x3', 'fused'),
                             (256, 768, 'bf16x3', 'stream')):
    assert route(33, n, s, prec, iters=16384)[0] == family
    assert route(33, n, s, prec, iters=16385)[0] == 'tiled'
    # an epsilon, 0.0 included, at each on-chip shape
    assert route(33, n, s, prec, eps=1e-3)[0] == 'tiled'
    assert route(33, n, s, prec, eps=0.0)[0] == 'tiled'
  assert route(33, 256, 512, 'bf16', iters=16385)[0] == 'refused'
  assert route(33, 256, 512, 'bf16', eps=0.0)[0] == 'refused'
  # both sides of gemm_prefers_small: more than 8 tiles of 128 x 128 and more
  # than one full tile per CU
  edge = frd.ceil_div(16384 * CUS, 200)
  assert route(edge - 1, 100, 200, 'f32')[3] == 'element'
  assert route(edge, 100, 200, 'f32')[3] == 'wide'
  assert route(edge, 100, 200, 'f32', cus=304)[3] == 'element'
  assert route(1024, 100, 128, 'f32', cus=4)[3] == 'element'      # 8 tiles
  assert route(1025, 100, 128, 'f32', cus=4)[3] == 'wide'         # 9 tiles
  # x3_want_slices equal to 1 and above
  assert frd.x3_want_slices(300, 64, 256) == 1
  assert route(300, 64, 256, 'f16x3')[2] == 'single'
  assert frd.x3_want_slices(300, 64, 257) == 2
  assert route(300, 64, 260, 'f16x3')[2] == 'split-k'
  # s % 4 (and n % 4): the wide epilogue in f32, a refusal on the splits
  assert route(edge + 1, 100, 201, 'f32')[3] == 'element'
  assert route(64, 100, 201, 'bf16x3')[0] == 'refused'
  assert route(64, 102, 200, 'f16x3')[0] == 'refused'
  assert route(64, 100, 200, 'f16x3') == ('tiled', 'f16', 'single', 'wide')


def test_round_bf16_is_nearest_even():
  x = np.concatenate([helpers.gaussian_patches(3, 64, 64).ravel(),
                      np.float32([1.00390625, 1.01171875, -1.00390625, 0.,
                                  1.0039062, 1.0039063])])
  want = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
  assert np.array_equal(frd.round_bf16(x), want.astype(np.float64))


@pytest.mark.parametrize('threshold', sorted(frd.THRESHOLDS))
@pytest.mark.parametrize('variant', ['fista', 'ista'])
def test_numpy_iteration_matches_oracle(variant, threshold):
  p = frd.problem('4 f32 element s=201', CUS)
  rows = p.rows[:40]
  init = frd.oracle(p, torch.float64, 2, rows=rows).numpy()
  for start in (None, init):
    kw = {} if start is None else {'initial_codes': torch.from_numpy(start)}
    ref = frd.oracle(p, torch.float64, frd.T, variant, rows, threshold,
                     **kw).numpy()
    own, pres = frd.iterates(p.X[rows], p.D, p.eta, p.case.lam, frd.T, variant,
                             threshold, start)
    assert len(pres) == frd.T
    assert np.array_equal(own != 0, ref != 0)
    assert helpers.rel_err(own, ref) < 1e-13


ALL_OPTIONS = [(c, 'fista') for c in frd.CASES] + [
    (c, o) for c, o in frd.OPTIONS if o != 'dev-eta']


@pytest.mark.parametrize('case,option', ALL_OPTIONS,
                         ids=['%s-%s' % (c.name, o) for c, o in ALL_OPTIONS])
def test_input_conditions(case, option):
  ref = frd.reference(case.name, CUS, option)
  frac, err, left_out = frd.assert_input_conditions(
      ref, '%s (%s)' % (case.name, option))
  print('%-44s %-24s T %3d  active %.2f  float32 %.2e  gate %.2e  left out '
        '%.3f' % (case.name, option, ref.spec.iters, frac, err, ref.gate[0],
                  left_out))
  if ref.spec.stop:
    assert len(ref.rows) == frd.problem(case.name, CUS).b
    assert 1 < ref.count < frd.STOP_ITERS
  if 'hard' in ref.spec.threshold:
    assert case.s <= 1024
    if ref.route[1] == 'bf16x2':
      assert case.s <= 256 or case.n < 256


def _faulty(p, ref, fault):
  return frd.iterates(
      p.X[ref.rows], p.D, p.eta, p.case.lam, ref.spec.iters, ref.spec.variant,
      ref.spec.threshold, None if ref.init is None else ref.init[ref.rows],
      'bf16' if ref.route[1] == 'bf16' else None, fault)[0]


@pytest.mark.parametrize('name', GATED)
def test_gates_catch_kernel_faults(name):
  p = frd.problem(name, CUS)
  missed = []
  for fault in frd.FAULTS:
    ref = frd.reference(name, CUS, FAULT_OPTION[fault])
    tol, flip = ref.gate
    keep = ref.keep
    # the iteration without the fault, rounded to float32, passes
    good = _faulty(p, ref, None).astype(np.float32)
    helpers.assert_codes_match(good[keep], ref.ref64[keep], tol, name,
                               max_flip_mag=flip)
    bad = _faulty(p, ref, fault).astype(np.float32)
    print('%-32s %-40s rel %.2e (gate %.1e)' % (
        name, fault, helpers.rel_err(bad[keep], ref.ref64[keep]), tol))
    try:
      helpers.assert_codes_match(bad[keep], ref.ref64[keep], tol, fault,
                                 max_flip_mag=flip)
      missed.append(fault)
    except AssertionError:
      pass
  assert not missed, missed


@pytest.mark.parametrize('name', ['4 f32 element s=201', '5 f16x3 split-K'])
def test_stop_count_catches_a_summed_change(name):
  """Early stopping compares the mean change per component; a kernel that
  compares the sum never stops inside STOP_ITERS."""
  p = frd.problem(name, CUS)
  ref = frd.reference(name, CUS, 'stop')
  assert frd.stop_count_numpy(p, p.case.stop_eps, np.mean) == ref.count
  assert frd.stop_count_numpy(p, p.case.stop_eps, np.sum) != ref.count
