"""The schedules of the fused FISTA kernel on 16x16x32 MFMAs
(csrc/fc_fused.hip, fused_fista_kernel16<..., SCHED>): bit 0 spreads the
epilogue of the middle phases over step 3 and step 1, bit 1 starts the residual
exchange under the iteration's last step 3.  A schedule moves work between
stream segments and changes no arithmetic, so the codes of every schedule are
those of schedule 0 bit for bit.  VTC_FUSED_SCHED=0|1|2|3 forces one; the
library reads it on every call."""
import numpy as np
import pytest
import torch

import helpers
import sc_oracle
from test_fc_fused_tile_gpu import (ETA, INDEX_RUNS, LAM, _integer_inputs,
                                    _restate_float64)

pytestmark = pytest.mark.gpu

SCHEDULES = ('0', '1', '2', '3')
# (nonnegative_only, hard_threshold)
THRESHOLDS = [(False, False), (True, False), (False, True), (True, True)]
# (variant, iterations)
ITERATIONS = [('fista', 1), ('fista', 2), ('fista', 7), ('ista', 2)]
# (precision, tile to force): f16x3 and bf16 run the 16x16x32 tile by default,
# bf16x3 only by force
PRECISIONS = [('f16x3', None), ('bf16', None), ('bf16x3', '16')]


@pytest.fixture(scope='module')
def ista_fista():
  from analysis_transforms.fully_connected import ista_fista
  if not ista_fista.fused_available():
    pytest.fail('libvtc_hip.so was built without the fused FISTA kernel')
  return ista_fista


@pytest.fixture
def sched(monkeypatch):
  def force(which, tile=None):
    monkeypatch.setenv('VTC_FUSED_SCHED', which)
    if tile is None:
      monkeypatch.delenv('VTC_FUSED_TILE', raising=False)
    else:
      monkeypatch.setenv('VTC_FUSED_TILE', tile)
  return force


# ----------------------------------------------------- 1. bitwise equality
@pytest.mark.parametrize('prec,tile', PRECISIONS)
@pytest.mark.parametrize('s', [256, 512, 1024])
def test_schedules_give_the_same_bits(device, ista_fista, sched, s, prec, tile):
  """Schedule 0 against 1, 2 and 3: two, four and eight phases (no middle
  phase, two, six), ragged last workgroups with dead lanes, FISTA and ISTA,
  cold and warm start, the four thresholds."""
  D = helpers.to_dev(helpers.unit_rows(41 + s, s, 256), device)
  eta = float(sc_oracle.fc_stepsize(D.cpu()))
  for b in (1, 31, 33, 69):
    X = helpers.to_dev(helpers.gaussian_patches(40 + b, b, 256), device)
    rs = np.random.RandomState(7 * b + s)
    init = helpers.to_dev(
        (0.05 * rs.randn(b, s) * (rs.rand(b, s) < 0.1)).astype(np.float32),
        device)
    for variant, iters in ITERATIONS:
      for start in (None, init):
        for nonneg, hard in THRESHOLDS:
          outs = []
          for which in SCHEDULES:
            sched(which, tile)
            outs.append(ista_fista.run(
                X, D, 0.02, iters, variant=variant, precision=prec,
                stepsize=eta, nonnegative_only=nonneg, hard_threshold=hard,
                initial_codes=start))
          what = (b, variant, iters, start is not None, nonneg, hard)
          assert bool(torch.isfinite(outs[0]).all()), what
          assert float(outs[0].abs().max()) > 0, what
          for which, out in zip(SCHEDULES[1:], outs[1:]):
            assert torch.equal(out, outs[0]), what + (which,)


# ------------------------------------------------------------ 2. range guard
def test_schedules_agree_when_the_range_guard_fires(device, ista_fista, sched):
  """f16x3 with a caller's stepsize of 4 / L: the iteration diverges, the
  scaled residual passes the guard's 2048 and the kernel rescales its state
  over and over.  Schedules 2 and 3 reorder the code around the guard.  ISTA:
  in 60 iterations the oracle's codes grow by 10^27 and stay finite (FISTA's
  overflow f32)."""
  Xn = helpers.gaussian_patches(900, 33, 256)
  Dn = helpers.unit_rows(901, 512, 256)
  Xc, Dc = torch.from_numpy(Xn), torch.from_numpy(Dn)
  eta = 4.0 * float(sc_oracle.fc_stepsize(Dc))
  ref, trace = sc_oracle.fc_ista_fista(Xc, Dc, 0.02, 60, variant='ista',
                                       stepsize=eta, trace_at=[1, 60])
  assert bool(torch.isfinite(ref).all())
  growth = float(trace[60].abs().max() / trace[1].abs().max())
  assert growth > 2.0 ** 4, growth
  X, D = helpers.to_dev(Xn, device), helpers.to_dev(Dn, device)
  outs = []
  for which in SCHEDULES:
    sched(which)
    outs.append(ista_fista.run(X, D, 0.02, 60, variant='ista',
                               precision='f16x3', stepsize=eta))
  assert bool(torch.isfinite(outs[0]).all())
  # the kernel followed the oracle up: the guard had to fire on the way
  assert float(outs[0].abs().max()) > 2.0 ** 4 * float(trace[1].abs().max())
  for which, out in zip(SCHEDULES[1:], outs[1:]):
    assert torch.equal(out, outs[0]), which


# -------------------------------------------------------------- 3. lane maps
@pytest.mark.parametrize('s', [256, 512, 1024])
def test_index_maps_exactly_under_both_parts(device, ista_fista, sched, s):
  """The integer-input cases of test_fc_fused_tile_gpu.py (every product and
  sum exact in f32, so the codes equal the oracle's bit for bit and any mistake
  in a lane map shows) on the 16x16x32 tile under schedule 3."""
  for b in (1, 31, 33, 69):
    Xn, Dn = _integer_inputs(b, s)
    Xc, Dc = torch.from_numpy(Xn), torch.from_numpy(Dn)
    X, D = helpers.to_dev(Xn, device), helpers.to_dev(Dn, device)
    i = np.arange(b)[:, None]
    a = np.arange(s)[None, :]
    warm = (((i + 3 * a) % 4 - 1) * ((i + a) % 3 == 0) * 0.25).astype(
        np.float32)
    for variant, iters, warm_start in INDEX_RUNS:
      init = warm if warm_start else None
      want64 = _restate_float64(Xn, Dn, iters, variant == 'fista', init, 16)
      ref = sc_oracle.fc_ista_fista(
          Xc, Dc, LAM, iters, variant=variant, stepsize=ETA,
          initial_codes=None if init is None else torch.from_numpy(init))
      assert np.array_equal(ref.numpy().astype(np.float64), want64)
      assert np.any(want64)
      precisions = ['f16x3', 'bf16x3']
      if iters == 1 and not warm_start:
        _restate_float64(Xn, Dn, iters, variant == 'fista', init, 8)
        precisions.append('bf16')
      for prec in precisions:
        sched('3', '16')
        out = ista_fista.run(
            X, D, LAM, iters, variant=variant, precision=prec, stepsize=ETA,
            initial_codes=None if init is None else helpers.to_dev(
                init, device))
        assert torch.equal(out.cpu(), ref), (b, variant, iters, warm_start,
                                             prec)


# ---------------------------------------------------------- 4. repeatability
@pytest.mark.parametrize('which', [None, '1', '2', '3'])
def test_schedule_repeats_bit_for_bit(device, ista_fista, monkeypatch, which):
  """626 workgroups, the last one ragged, 20 runs of whatever schedule the
  library picks (None) and of each forced one: a race between an early
  publication and a late reader would show as a run that differs."""
  if which is None:
    monkeypatch.delenv('VTC_FUSED_SCHED', raising=False)
  else:
    monkeypatch.setenv('VTC_FUSED_SCHED', which)
  monkeypatch.delenv('VTC_FUSED_TILE', raising=False)
  X = helpers.to_dev(helpers.gaussian_patches(50, 20001, 256), device)
  D = helpers.to_dev(helpers.unit_rows(51, 1024, 256), device)
  eta = float(sc_oracle.fc_stepsize(D.cpu()))
  first = ista_fista.run(X, D, 0.02, 12, precision='f16x3', stepsize=eta)
  assert float(first.abs().max()) > 0
  for _ in range(19):
    again = ista_fista.run(X, D, 0.02, 12, precision='f16x3', stepsize=eta)
    assert torch.equal(again, first)
