"""CPU checks behind tests/test_update_routes_gpu.py: the float64 restatement
in update_oracle.py agrees with sc_oracle, every step gate catches a 1e-4
relative gradient error, and the dictionary-level gates of the older update
tests do not.  No GPU needed."""
import numpy as np
import pytest
import torch

import helpers
import sc_oracle
import update_oracle as uo


def _conv_problem(seed, c, kh, kw, stride, s, b, height, width):
  rs = np.random.RandomState(seed)
  lead_v, trail_v = sc_oracle.conv_padding_amount(height, kh, stride[0])
  lead_h, trail_h = sc_oracle.conv_padding_amount(width, kw, stride[1])
  x = np.zeros((b, c, height + lead_v + trail_v, width + lead_h + trail_h))
  x[:, :, lead_v:lead_v + height, lead_h:lead_h + width] = 0.5 * rs.randn(
      b, c, height, width)
  d = rs.randn(s, c, kh, kw)
  d /= np.sqrt((d ** 2).sum(axis=(1, 2, 3)))[:, None, None, None]
  ch = sc_oracle.conv_code_dim(x.shape[2], kh, stride[0])
  cw = sc_oracle.conv_code_dim(x.shape[3], kw, stride[1])
  codes = 0.05 * rs.randn(b, s, ch, cw) * (rs.rand(b, s, ch, cw) < 0.2)
  pad = ((lead_v, trail_v), (lead_h, trail_h))
  return (torch.from_numpy(x), torch.from_numpy(d), torch.from_numpy(codes),
          pad)


def _fc_problem(seed, b, n, s):
  rs = np.random.RandomState(seed)
  x = torch.from_numpy(0.1 * rs.randn(b, n))
  d = rs.randn(s, n)
  d = torch.from_numpy(d / np.linalg.norm(d, axis=1, keepdims=True))
  codes = torch.from_numpy(0.05 * rs.randn(b, s) * (rs.rand(b, s) < 0.2))
  h = torch.from_numpy(0.01 + 0.05 * rs.rand(s))
  return x, d, codes, h


CONV_GEOMETRIES = [(1, 5, 5, (1, 1), 6, 2, 13, 11),
                   (2, 5, 7, (1, 1), 5, 3, 12, 15),
                   (3, 6, 6, (2, 2), 4, 2, 11, 14),
                   (2, 6, 4, (3, 2), 7, 3, 16, 13),
                   (1, 16, 16, (2, 2), 3, 2, 20, 22)]


@pytest.mark.parametrize('geom', CONV_GEOMETRIES)
def test_conv_gradient_sum_matches_oracle(geom):
  c, kh, kw, stride, s, b, height, width = geom
  x, d, codes, pad = _conv_problem(7, c, kh, kw, stride, s, b, height, width)
  ours = uo.conv_gradient_sum(x, d, codes, stride, pad)
  ref = sc_oracle.conv_gradient(x, d, codes, stride, pad) * b
  assert uo.rel(ours, ref) < 1e-13
  if kh * kw <= 35:
    naive = sc_oracle.conv_gradient_naive(x, d, codes, stride, pad) * b
    assert uo.rel(ours, naive) < 1e-13


@pytest.mark.parametrize('hessian', [False, True])
def test_conv_apply_matches_oracle(hessian):
  x, d0, codes, pad = _conv_problem(8, 2, 6, 6, (2, 2), 5, 2, 15, 12)
  h = torch.linspace(0.01, 0.06, 5, dtype=torch.float64)
  g = uo.conv_gradient_sum(x, d0, codes, (2, 2), pad)
  ours = uo.conv_apply(d0, g, 2, 0.03, h if hessian else None)
  ref = d0.clone()
  if hessian:
    sc_oracle.conv_cheap_quadratic_descent(x, ref, codes, h, (2, 2), pad,
                                           stepsize=0.03)
  else:
    sc_oracle.conv_steepest_descent(x, ref, codes, (2, 2), pad,
                                    stepsize=0.03)
  assert uo.rel(ours, ref) < 1e-14


@pytest.mark.parametrize('normalize', [True, False])
def test_fc_apply_matches_oracle(normalize):
  x, d0, codes, h = _fc_problem(9, 40, 12, 10)
  g = uo.fc_gradient_sum(x, d0, codes)
  ref = d0.clone()
  sc_oracle.fc_steepest_descent(x, ref, codes, stepsize=0.3,
                                normalize_dictionary=normalize)
  assert uo.rel(uo.fc_apply(d0, g, 40, 0.3, normalize=normalize), ref) < 1e-14
  ref = d0.clone()
  sc_oracle.fc_cheap_quadratic_descent(x, ref, codes, h, stepsize=0.3,
                                       normalize_dictionary=normalize)
  assert uo.rel(uo.fc_apply(d0, g, 40, 0.3, h, normalize=normalize),
                ref) < 1e-14
  groups = [[0, 1, 2], [3, 4], [5, 6, 7, 8, 9], [2, 5]]
  ref = d0.clone()
  sc_oracle.subspace_cheap_quadratic_descent(
      x, ref, codes, groups, h, 0.05, stepsize=0.3,
      normalize_dictionary=normalize)
  p = uo.alignment_gradient_sum(d0, groups, normalize)
  assert uo.rel(uo.fc_apply(d0, g, 40, 0.3, h, p, 0.05, normalize),
                ref) < 1e-14


@pytest.mark.parametrize('normalize', [True, False])
def test_alignment_fallback_matches_oracle(normalize):
  """The float64 fallback of the subspace plugin for groups past the kernel's
  LDS tile, against the oracle's per-group loop: ragged and overlapping
  groups, un-normalised rows."""
  from dict_update_rules.fully_connected import (
      subspace_sc_cheap_quadratic_descent as plugin)
  rs = np.random.RandomState(10)
  d = torch.from_numpy(rs.randn(20, 9) * rs.uniform(0.5, 2.0, (20, 1)))
  groups = [[0, 1, 2, 3, 4, 5, 6], [7], [8, 9, 10], [11, 12, 13, 14, 15],
            [16, 17, 18, 19], [3, 8, 16]]
  ours = plugin.alignment_gradient_float64(d.float(), groups, normalize)
  ref = uo.alignment_gradient_sum(d.float(), groups, normalize)
  assert ours.dtype == torch.float32
  assert uo.rel(ours, ref) < 1e-7


def test_alignment_device_limits():
  """Which groups the alignment kernel takes (csrc/dict_update.hip)."""
  from dict_update_rules.fully_connected import (
      subspace_sc_cheap_quadratic_descent as plugin)
  fits = plugin.alignment_fits_device
  assert fits(8, 16) and fits(32, 64) and fits(32, 576)
  assert fits(64, 256) and fits(128, 64)
  assert not fits(64, 640)          # 176 KiB tile
  assert not fits(200, 8)           # 163 KiB: the m^2 cosine table
  assert not fits(257, 1)           # one thread per member


def test_gradient_gates_catch_perturbation():
  g = torch.from_numpy(np.random.RandomState(11).randn(30, 17))
  bad = uo.perturb(g, uo.PERTURBATION)
  assert abs(uo.rel(bad, g) - uo.PERTURBATION) < 1e-12
  for name, gate in uo.GRAD_GATES.items():
    assert uo.PERTURBATION > 3 * gate, name


def _fc_step_errors():
  """Step error of a 1e-4 gradient error, per FC-family update rule."""
  x, d0, codes, h = _fc_problem(12, 64, 20, 24)
  g = uo.fc_gradient_sum(x, d0, codes)
  bad = uo.perturb(g, uo.PERTURBATION)
  out = {}
  for name, hess in (('steepest', None), ('cheapquad', h)):
    for normalize in (True, False):
      eta = uo.fc_stepsize(d0, g, 64, hess)
      ref = uo.fc_apply(d0, g, 64, eta, hess, normalize=normalize)
      assert uo.step_fraction(ref, d0) >= uo.MIN_STEP_FRACTION
      ours = uo.fc_apply(d0, bad, 64, eta, hess, normalize=normalize)
      out[(name, normalize)] = uo.step_error(ours, ref, d0)
  return out


def test_fc_step_gate_catches_gradient_error():
  for key, err in _fc_step_errors().items():
    assert err > uo.STEP_GATES['fc'], (key, err)


def test_subspace_step_gate_catches_gradient_error():
  """Penalty 0: an error in the data term; penalty 0.05: an error in the
  alignment gradient, which then dominates the step."""
  x, d0, codes, h = _fc_problem(13, 64, 20, 24)
  groups = [list(range(k, k + 6)) for k in range(0, 24, 6)]
  g = uo.fc_gradient_sum(x, d0, codes)
  for normalize in (True, False):
    eta = uo.fc_stepsize(d0, g, 64, h)
    ref = uo.fc_apply(d0, g, 64, eta, h, normalize=normalize)
    ours = uo.fc_apply(d0, uo.perturb(g, uo.PERTURBATION), 64, eta, h,
                       normalize=normalize)
    err = uo.step_error(ours, ref, d0)
    assert err > uo.STEP_GATES['subspace'], (normalize, err)
    p = uo.alignment_gradient_sum(d0, groups, normalize)
    eta = uo.fc_stepsize(d0, g, 64, h, p, 0.05)
    ref = uo.fc_apply(d0, g, 64, eta, h, p, 0.05, normalize)
    assert uo.step_fraction(ref, d0) >= uo.MIN_STEP_FRACTION
    ours = uo.fc_apply(d0, g, 64, eta, h, uo.perturb(p, uo.PERTURBATION),
                       0.05, normalize)
    err = uo.step_error(ours, ref, d0)
    assert err > uo.STEP_GATES['subspace'], (normalize, err)


def test_conv_step_gates_catch_gradient_error():
  for geom in CONV_GEOMETRIES[:4]:
    c, kh, kw, stride, s, b, height, width = geom
    x, d0, codes, pad = _conv_problem(14, c, kh, kw, stride, s, b, height,
                                      width)
    h = torch.from_numpy(np.random.RandomState(15).uniform(0.01, 0.06, s))
    g = uo.conv_gradient_sum(x, d0, codes, stride, pad)
    bad = uo.perturb(g, uo.PERTURBATION)
    for hess in (None, h):
      ref = uo.conv_apply(d0, g, b, uo.STEP_FRACTION, hess)
      assert uo.step_fraction(ref, d0) >= uo.MIN_STEP_FRACTION
      err = uo.step_error(uo.conv_apply(d0, bad, b, uo.STEP_FRACTION, hess),
                          ref, d0)
      assert err > uo.STEP_GATES['conv-f32'], (geom, err)
      assert err > uo.STEP_GATES['conv-bf16x3'], (geom, err)


def test_dictionary_gates_miss_gradient_error():
  """Why the step is gated: at the step sizes of the older update tests a
  1e-4 gradient error stays under their gates on D (REL_TOL_DICT for the FC
  goldens, 5e-6 for the conv updates at eta = 0.005)."""
  g = helpers.load('fc_c1')
  x = torch.from_numpy(g['images']).double()
  codes = torch.from_numpy(g['codes_fista_soft']).double()
  d0 = torch.from_numpy(g['dictionary']).double()
  b = x.shape[0]
  grad = uo.fc_gradient_sum(x, d0, codes)
  ref = uo.fc_apply(d0, grad, b, 0.1)
  ours = uo.fc_apply(d0, uo.perturb(grad, uo.PERTURBATION), b, 0.1)
  assert uo.rel(ours, ref) < helpers.REL_TOL_DICT
  assert uo.step_error(ours, ref, d0) > uo.STEP_GATES['fc']
  x, d0, codes, pad = _conv_problem(16, 1, 11, 11, (1, 1), 32, 2, 30, 34)
  grad = uo.conv_gradient_sum(x, d0, codes, (1, 1), pad)
  ref = uo.conv_apply(d0, grad, 2, 0.005)
  ours = uo.conv_apply(d0, uo.perturb(grad, uo.PERTURBATION), 2, 0.005)
  assert uo.rel(ours, ref) < 5e-6
  assert uo.step_error(ours, ref, d0) > uo.STEP_GATES['conv-bf16x3']
