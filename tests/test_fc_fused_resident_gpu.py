"""Schedule bit 2 of the fused FISTA kernel on 16x16x32 MFMAs and its
compiled-in variant (csrc/fc_fused.hip, fused_fista_kernel16<..., SCHED,
FISTA>).

Bit 2 keeps the B operands of step 1's first k-steps -- the residual, which is
the same in every phase of an iteration -- in registers instead of reading them
from the exchange image in every phase.  It changes no operand, no product and
no summation order, so the codes of schedules 4..7 are those of schedule 0 bit
for bit.  VTC_FUSED_SCHED=0..7 forces a schedule; the library reads it on every
call.

The variant (FISTA or ISTA) is a template argument of that kernel, where it was
a run-time select; the lo part of the f16 split is subtracted per element, where
it was subtracted in pairs.  Neither changes a value: the codes of schedules
0..3 and of the 32x32x16 kernel are compared with digests of the codes the
parent commit's build gave on the same inputs (tests/golden/
fc_fused_parent_codes.npz).  They were recorded by running this file as a
script, `python tests/test_fc_fused_resident_gpu.py OUT.npz`, on an MI355X with
the parent commit's libvtc_hip.so in place of the package's; the kernel is
deterministic (no atomics; test_fc_fused_sched_gpu.py repeats it bit for bit)."""
import hashlib
import pathlib
import sys

import numpy as np
import pytest
import torch

if __name__ == '__main__':
  _REPO = pathlib.Path(__file__).resolve().parent.parent
  for _p in (_REPO / 'vision-transform-codes_amd', _REPO / 'oracle',
             _REPO / 'tests'):
    sys.path.insert(0, str(_p))

import helpers
import sc_oracle

pytestmark = pytest.mark.gpu

BASE = '0'
RESIDENT = ('4', '5', '7')
# (nonnegative_only, hard_threshold)
THRESHOLDS = [(False, False), (True, False), (False, True), (True, True)]
# (variant, iterations): T in {1, 2, 5}, both variants
ITERATIONS = [('fista', 1), ('fista', 2), ('fista', 5), ('ista', 2),
              ('ista', 5)]
# (precision, tile to force): f16x3 and bf16 run the 16x16x32 tile by default,
# bf16x3 only by force
PRECISIONS = [('f16x3', None), ('bf16', None), ('bf16x3', '16')]
# one full group; a second group with one live patch; a ragged last group
BATCHES = (32, 33, 95)
REL_TOL_BF16 = 5e-2     # the gate of test_fc_fused_gpu.py's bf16 fast mode


@pytest.fixture(scope='module')
def ista_fista():
  from analysis_transforms.fully_connected import ista_fista
  if not ista_fista.fused_available():
    pytest.fail('libvtc_hip.so was built without the fused FISTA kernel')
  return ista_fista


@pytest.fixture
def sched(monkeypatch):
  def force(which, tile=None):
    if which is None:
      monkeypatch.delenv('VTC_FUSED_SCHED', raising=False)
    else:
      monkeypatch.setenv('VTC_FUSED_SCHED', which)
    if tile is None:
      monkeypatch.delenv('VTC_FUSED_TILE', raising=False)
    else:
      monkeypatch.setenv('VTC_FUSED_TILE', tile)
  return force


# ----------------------------------------------------- 1. bitwise equality
@pytest.mark.parametrize('prec,tile', PRECISIONS)
@pytest.mark.parametrize('s', [256, 512, 1024])
def test_resident_schedules_give_the_bits_of_schedule_0(device, ista_fista,
                                                        sched, s, prec, tile):
  """Schedules 4, 5 and 7 against 0: two, four and eight phases (NPH = 2 has no
  middle phase), the three batch shapes, T in {1, 2, 5}, FISTA and ISTA, cold
  and warm start, the four thresholds."""
  D = helpers.to_dev(helpers.unit_rows(61 + s, s, 256), device)
  eta = float(sc_oracle.fc_stepsize(D.cpu()))
  for b in BATCHES:
    X = helpers.to_dev(helpers.gaussian_patches(60 + b, b, 256), device)
    rs = np.random.RandomState(11 * b + s)
    init = helpers.to_dev(
        (0.05 * rs.randn(b, s) * (rs.rand(b, s) < 0.1)).astype(np.float32),
        device)
    for variant, iters in ITERATIONS:
      for start in (None, init):
        for nonneg, hard in THRESHOLDS:
          outs = []
          for which in (BASE,) + RESIDENT:
            sched(which, tile)
            outs.append(ista_fista.run(
                X, D, 0.02, iters, variant=variant, precision=prec,
                stepsize=eta, nonnegative_only=nonneg, hard_threshold=hard,
                initial_codes=start))
          what = (b, variant, iters, start is not None, nonneg, hard)
          assert bool(torch.isfinite(outs[0]).all()), what
          assert float(outs[0].abs().max()) > 0, what
          for which, out in zip(RESIDENT, outs[1:]):
            assert torch.equal(out, outs[0]), what + (which,)


# ------------------------------------------------------------ 2. range guard
@pytest.mark.parametrize('variant,iters', [('ista', 60), ('fista', 24)])
def test_resident_operand_follows_the_range_guard(device, ista_fista, sched,
                                                  variant, iters):
  """The recipe of test_fc_fused_sched_gpu.py: f16x3 with a caller's stepsize
  of 4 / L, so that the iteration diverges, the scaled residual passes the
  guard's 2048 and the kernel rescales its state over and over.  The resident
  operand is read after the barrier that follows the rescaled publication: a
  copy taken before it, or at the wrong scale, would differ from schedule 0.
  That the guard fired is inferred as there: the codes followed the oracle up
  by more than 2^4, which the scaled units cannot hold without it."""
  Xn = helpers.gaussian_patches(900, 33, 256)
  Dn = helpers.unit_rows(901, 512, 256)
  Xc, Dc = torch.from_numpy(Xn), torch.from_numpy(Dn)
  eta = 4.0 * float(sc_oracle.fc_stepsize(Dc))
  ref, trace = sc_oracle.fc_ista_fista(Xc, Dc, 0.02, iters, variant=variant,
                                       stepsize=eta, trace_at=[1, iters])
  assert bool(torch.isfinite(ref).all())
  growth = float(trace[iters].abs().max() / trace[1].abs().max())
  assert growth > 2.0 ** 4, growth
  X, D = helpers.to_dev(Xn, device), helpers.to_dev(Dn, device)
  outs = []
  for which in (BASE,) + RESIDENT + ('6',):
    sched(which)
    outs.append(ista_fista.run(X, D, 0.02, iters, variant=variant,
                               precision='f16x3', stepsize=eta))
  assert bool(torch.isfinite(outs[0]).all())
  assert float(outs[0].abs().max()) > 2.0 ** 4 * float(trace[1].abs().max())
  for which, out in zip(RESIDENT + ('6',), outs[1:]):
    assert torch.equal(out, outs[0]), which


# ------------------------------------------------------- 3. against the oracle
@pytest.mark.parametrize('which', [None, '5', '7'])
def test_reference_codes_at_200_iterations(device, ista_fista, sched, which):
  """fc_c2_mini.npz, the reference's own codes after 200 FISTA steps, at the
  gates of test_fc_fused_gpu.py: through the library's default schedule and
  through the resident-operand schedules by force."""
  sched(which)
  g = helpers.load('fc_c2_mini')
  X = helpers.to_dev(helpers.gaussian_patches(0, 64, 256), device)
  D = helpers.to_dev(helpers.unit_rows(1, 1024, 256), device)
  lam, eta = float(g['sparsity_weight']), float(g['stepsize'])
  codes = ista_fista.run(X, D, lam, 200, precision='f16x3', stepsize=eta)
  err, flips = helpers.assert_codes_match(
      codes.cpu().numpy(), g['codes_fista_T200'], helpers.REL_TOL_F32,
      'f16x3 T=200 schedule %s' % which, max_flip_mag=helpers.NEAR_THRESHOLD)
  print('schedule %s fc_c2 f16x3 T=200 rel %.2e flips %d' % (which, err, flips))
  fast = ista_fista.run(X, D, lam, 200, precision='bf16', stepsize=eta)
  err = helpers.rel_err(fast.cpu().numpy(), g['codes_fista_T200'])
  print('schedule %s fc_c2 bf16 T=200 rel %.2e' % (which, err))
  assert err < REL_TOL_BF16


# ------------------------------------------- 4. the bits of the parent's build
PARENT_S, PARENT_B, PARENT_T, PARENT_LAM = 512, 33, 3, 0.02
# (precision, tile, schedules): every schedule the parent had
PARENT_ARMS = [(prec, '16', ('0', '1', '2', '3'))
               for prec in ('f16x3', 'bf16', 'bf16x3')] + \
              [(prec, '32', ('0',)) for prec in ('f16x3', 'bf16', 'bf16x3')]


def _parent_cases():
  for prec, tile, schedules in PARENT_ARMS:
    for which in schedules:
      for variant in ('fista', 'ista'):
        for nonneg, hard in THRESHOLDS:
          yield prec, tile, which, variant, nonneg, hard


def _parent_key(prec, tile, which, variant, nonneg, hard):
  return '%s_t%s_s%s_%s_%d%d' % (prec, tile, which, variant, nonneg, hard)


def _parent_digests(device, ista_fista, setenv):
  """sha256 of the codes (float32, C order) of every parent case: four phases
  (two middle ones), two workgroups, the second with one live patch.  A digest
  has no tolerance, so the inputs are exact on every host: seeded integers
  times a power of two (no libm, no host summation), and a stepsize that is a
  constant below 1 / L (rows of norm ~0.58, L ~ 2) instead of a host
  eigenvalue."""
  rs = np.random.RandomState(77)
  D = helpers.to_dev((rs.randint(-2 ** 11, 2 ** 11, size=(PARENT_S, 256)) *
                      2.0 ** -15).astype(np.float32), device)
  X = helpers.to_dev((rs.randint(-2 ** 15, 2 ** 15, size=(PARENT_B, 256)) *
                      2.0 ** -18).astype(np.float32), device)
  eta = 0.25
  out = {}
  for case in _parent_cases():
    prec, tile, which, variant, nonneg, hard = case
    setenv('VTC_FUSED_TILE', tile)
    setenv('VTC_FUSED_SCHED', which)
    codes = ista_fista.run(X, D, PARENT_LAM, PARENT_T, variant=variant,
                           precision=prec, stepsize=eta,
                           nonnegative_only=nonneg, hard_threshold=hard)
    codes = np.ascontiguousarray(codes.cpu().numpy(), dtype=np.float32)
    assert np.isfinite(codes).all() and np.abs(codes).max() > 0, case
    out[_parent_key(*case)] = np.frombuffer(
        hashlib.sha256(codes.tobytes()).digest(), dtype=np.uint8)
  return out


def test_schedules_0_to_3_and_the_other_tile_give_the_parents_bits(
    device, ista_fista, monkeypatch):
  g = helpers.load('fc_fused_parent_codes')
  want = dict(zip(g['keys'].tolist(), g['digests']))
  got = _parent_digests(device, ista_fista, monkeypatch.setenv)
  assert sorted(got) == sorted(want)
  differ = [k for k in sorted(got) if not np.array_equal(got[k], want[k])]
  assert not differ, differ


if __name__ == '__main__':
  import os

  def _setenv(name, value):
    os.environ[name] = value

  from analysis_transforms.fully_connected import ista_fista as _plugin
  _got = _parent_digests(torch.device('cuda:0'), _plugin, _setenv)
  _keys = sorted(_got)
  np.savez_compressed(sys.argv[1], keys=np.array(_keys),
                      digests=np.stack([_got[k] for k in _keys]))
  print('recorded', len(_keys), 'digests to', sys.argv[1])
