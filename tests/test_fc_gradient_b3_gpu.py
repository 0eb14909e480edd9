"""vtc_fc_dict_gradient on the three-part bf16 route (csrc/gemm_b3.h).

Every case forces a route with VTC_FC_GRAD and asserts, through a Python
mirror of fc_gradient_b3_usable, which one that call takes.  Exact cases use
inputs whose every partial sum is representable in float32, so the result must
equal float64 bit for bit; the gated cases use the gates of update_oracle.py.
Measured errors: profiles/fc_gradient_b3.txt."""
import numpy as np
import pytest
import torch

import helpers
import update_oracle as uo
from test_update_routes_gpu import _fc_problem

pytestmark = pytest.mark.gpu

ceil_div = lambda a, b: -(-a // b)
B_MIN = 1024            # kB3MinBatch
SMALLEST = (B_MIN, 64, 64)


def _gradient_slices(b, n, s):
  """gradient_slices (csrc/dict_update.hip)."""
  want = ceil_div(1024, ceil_div(s, 128) * ceil_div(n, 128))
  want = max(1, min(want, ceil_div(b, 64), 128))
  chunk = max(16, ceil_div(ceil_div(b, want), 16) * 16)
  return ceil_div(b, chunk)


def _b3_usable(tensors, b, n, s):
  """fc_gradient_b3_usable (csrc/gemm_b3.h)."""
  if any(t.data_ptr() % 16 for t in tensors):
    return False
  if n % 64 or s % 64 or b < B_MIN:
    return False
  slices = _gradient_slices(b, n, s)
  chunk = ceil_div(ceil_div(b, slices), 16) * 16
  return max(chunk, 128) * max(n, s) * 4 < 0x7fffffff


def _b3_faster(b, n, s):
  """fc_gradient_b3_faster (csrc/gemm_b3.h): the default past the cut-over."""
  return b >= 8192 and b * n * s >= 2 ** 31


def _gradient(X, D, C, force, monkeypatch, expect, out=None):
  """grad_sum under VTC_FC_GRAD=force (None: unset, the default route);
  `expect` is the route it must take."""
  import vtc_hip
  lib = vtc_hip.load_library()
  b, n = X.shape
  s = D.shape[0]
  if out is None:
    out = torch.empty(s, n, device=X.device)
  want = force or ('b3' if _b3_faster(b, n, s) else 'f32')
  took = want if _b3_usable((X, D, C, out), b, n, s) else 'f32'
  assert took == expect
  if force:
    monkeypatch.setenv('VTC_FC_GRAD', force)
  else:
    monkeypatch.delenv('VTC_FC_GRAD', raising=False)
  ws = vtc_hip.workspace(lib.vtc_fc_dict_gradient_workspace_bytes(b, n, s),
                         X.device)
  vtc_hip.check(lib.vtc_fc_dict_gradient(
      vtc_hip.ptr(X), vtc_hip.ptr(D), vtc_hip.ptr(C), vtc_hip.ptr(out), b, n,
      s, vtc_hip.ptr(ws), ws.numel(), vtc_hip.current_stream(X.device)),
      'vtc_fc_dict_gradient')
  return out


def _exact(grad, X, D, C):
  # (not uo.fc_gradient_sum: that divides by b and multiplies it back, which
  # rounds in float64 unless b is a power of two)
  X, D, C = X.double(), D.double(), C.double()
  ref = C.t() @ (C @ D - X)
  bad = int((grad.double() != ref).sum())
  assert bad == 0, '%d of %d entries differ from float64, worst %.3e' % (
      bad, ref.numel(), float((grad.double() - ref).abs().max()))


# ------------------------------------------------------- lane maps, part order
@pytest.mark.parametrize('shape', [SMALLEST, (B_MIN + 33, 256, 256)],
                         ids=['one-tile', '2x2-tiles-ragged-slabs'])
def test_small_integers_are_exact(device, monkeypatch, shape):
  """C in {-3..3} at 20 % density, D and X in {-4..4}: every partial sum is an
  integer below 2^24, so any lane, tile, part or slab mix-up shows."""
  b, n, s = shape
  assert _gradient_slices(b, n, s) >= 2
  rs = np.random.RandomState(b + n)
  C = rs.randint(-3, 4, (b, s)) * (rs.rand(b, s) < 0.2)
  D = rs.randint(-4, 5, (s, n))
  X = rs.randint(-4, 5, (b, n))
  assert 3 * (12 * s + 4) * b < 2 ** 24
  X, D, C = (helpers.to_dev(a.astype(np.float32), device) for a in (X, D, C))
  _exact(_gradient(X, D, C, 'b3', monkeypatch, 'b3'), X, D, C)


# ------------------------------------------------- every part, every product
def _live_case(kind, b, n, s):
  """One non-zero code per atom (in a row of its own), so that each entry of
  E and of G is a single product; the values are chosen so that it is exact
  in float32 only if the named part products are formed (the others the case
  needs are listed).  c: the code, d: the dictionary row, X is set so that
  E = C D - X has the parts the second product is to see."""
  rs = np.random.RandomState(len(kind) + ord(kind[0]) + 7 * ord(kind[1]))
  rows = rs.permutation(b)[:s]
  pow2 = lambda shape: np.ldexp(rs.choice([-1.0, 1.0], shape),
                                rs.randint(-3, 4, shape))
  odd = lambda bits, shape: np.ldexp(
      rs.choice([-1.0, 1.0], shape) *
      (rs.randint(2 ** (bits - 2), 2 ** (bits - 1), shape) * 2 + 1), 3 - bits)
  c_unit = pow2(s)
  d_unit = pow2((s, n))
  if kind == 'hm':       # both products: hh, hm
    c, d, e = c_unit, odd(16, (s, n)), None
  elif kind == 'hl':     # both products: hh, hm, hl
    c, d, e = c_unit, odd(24, (s, n)), None
  elif kind == 'mh':     # both products: hh, mh
    c, d = c_unit * (1 + 2.0 ** -10), d_unit
    e = c_unit[:, None] * d
  elif kind == 'lh':     # both products: hh, mh, lh
    c, d = c_unit * (1 + 2.0 ** -9 + 2.0 ** -20), d_unit
    e = c_unit[:, None] * d
  else:                  # 'mm', both products: hh, hm, mh, mm
    c, d = c_unit * (1 + 2.0 ** -10), d_unit * (1 + 2.0 ** -10)
    e = c_unit[:, None] * d
  C = np.zeros((b, s))
  C[rows, np.arange(s)] = c
  X = np.zeros((b, n))
  if e is not None:
    X[rows] = c[:, None] * d - e
  for a in (C, d, X):
    assert (a.astype(np.float32) == a).all()
  return X.astype(np.float32), d.astype(np.float32), C.astype(np.float32)


@pytest.mark.parametrize('kind', ['hm', 'mh', 'hl', 'lh', 'mm'])
def test_each_part_product_is_live(device, monkeypatch, kind):
  b, n, s = B_MIN + 33, 64, 128
  X, D, C = (helpers.to_dev(a, device) for a in _live_case(kind, b, n, s))
  _exact(_gradient(X, D, C, 'b3', monkeypatch, 'b3'), X, D, C)


# ------------------------------------------------------------------ the gates
def _zero_blocks(C):
  C = C.clone()
  C.view(-1, 32, C.shape[1])[::2] = 0      # every other 32-row block
  return C


GATE_CASES = [
    ('smallest', SMALLEST, None),
    ('smallest+1', (B_MIN + 1, 64, 64), None),
    ('smallest+31', (B_MIN + 31, 64, 64), None),
    ('smallest+33', (B_MIN + 33, 64, 64), None),
    ('2048x256x1024', (2048, 256, 1024), None),
    ('8192x256x1024', (8192, 256, 1024), None),
    ('zero 32-row blocks', (2048, 128, 192), 'zero-blocks'),
    ('dense codes', (2048, 128, 192), 'dense'),
]


@pytest.mark.parametrize('case', GATE_CASES, ids=[c[0] for c in GATE_CASES])
def test_gradient_and_steps_within_the_gates(device, monkeypatch, case):
  from dict_update_rules.fully_connected import sc_steepest_descent
  from dict_update_rules.fully_connected import sc_cheap_quadratic_descent
  name, (b, n, s), codes = case
  X, D0, C, h = _fc_problem(device, 300 + n + b % 64, b, n, s)
  if codes == 'zero-blocks':
    C = _zero_blocks(C)
  elif codes == 'dense':
    rs = np.random.RandomState(5)
    C = helpers.to_dev((0.05 * rs.randn(b, s)).astype(np.float32), device)
  ref_grad = uo.fc_gradient_sum(X, D0, C)
  grad = _gradient(X, D0, C, 'b3', monkeypatch, 'b3')
  grad_f32 = _gradient(X, D0, C, 'f32', monkeypatch, 'f32')
  errs = {'b3': uo.rel(grad, ref_grad), 'f32': uo.rel(grad_f32, ref_grad),
          'b3-f32': uo.rel(grad, grad_f32)}
  monkeypatch.setenv('VTC_FC_GRAD', 'b3')
  assert _b3_usable((X, D0, C), b, n, s)
  for rule, hess in (('steepest', None), ('cheapquad', h)):
    eta = uo.fc_stepsize(D0, ref_grad, b, hess)
    ref = uo.fc_apply(D0, ref_grad, b, eta, hess)
    D = D0.clone()
    if hess is None:
      sc_steepest_descent.run(X, D, C, stepsize=eta)
    else:
      sc_cheap_quadratic_descent.run(X, D, C, hess, stepsize=eta)
    errs[rule] = uo.step_error(D, ref, D0)
  print('%-22s %s' % (name, '  '.join('%s %.2e' % kv
                                      for kv in sorted(errs.items()))))
  gate = uo.GRAD_GATES['fc-split-k']
  assert errs['b3'] < gate
  assert errs['b3-f32'] < 2 * gate
  assert errs['steepest'] < uo.STEP_GATES['fc']
  assert errs['cheapquad'] < uo.STEP_GATES['fc']


# ------------------------------------------------------------- exact scaling
@pytest.mark.parametrize('power', [20, -20])
def test_power_of_two_scaling_is_exact(device, monkeypatch, power):
  """bf16 parts carry the float32 exponent: C and X times 2^p gives E times
  2^p and G times 2^2p, bit for bit."""
  b, n, s = B_MIN + 33, 64, 128
  X, D, C, _ = _fc_problem(device, 41, b, n, s)
  base = _gradient(X, D, C, 'b3', monkeypatch, 'b3')
  scaled = _gradient(X * 2.0 ** power, D, C * 2.0 ** power, 'b3', monkeypatch,
                     'b3')
  assert torch.isfinite(scaled).all() and float(scaled.abs().max()) > 0
  assert torch.equal(scaled, base * 2.0 ** (2 * power))


# ----------------------------------------------------------- reproducibility
def test_twenty_runs_are_bitwise_equal(device, monkeypatch):
  b, n, s = 20001, 128, 256
  X, D, C, _ = _fc_problem(device, 43, b, n, s)
  first = _gradient(X, D, C, 'b3', monkeypatch, 'b3').clone()
  for _ in range(19):
    assert torch.equal(_gradient(X, D, C, 'b3', monkeypatch, 'b3'), first)


# ------------------------------------------------------ default and cut-over
@pytest.mark.parametrize('shape,route', [((8192, 256, 1024), 'b3'),
                                         ((4096, 256, 1024), 'f32'),
                                         ((8192, 256, 256), 'f32')])
def test_default_route_follows_the_cut_over(device, monkeypatch, shape, route):
  b, n, s = shape
  X, D, C, _ = _fc_problem(device, 45, b, n, s)
  default = _gradient(X, D, C, None, monkeypatch, route).clone()
  assert torch.equal(default, _gradient(X, D, C, route, monkeypatch, route))


# ------------------------------------------------------------------ fallbacks
@pytest.mark.parametrize('what', ['offset-view', 'n=12', 'b=200'])
def test_forced_b3_falls_back_to_f32(device, monkeypatch, what):
  """Where the preconditions fail a forced b3 is today's route, bit for bit."""
  b, n, s = {'offset-view': (B_MIN, 64, 64), 'n=12': (B_MIN, 12, 64),
             'b=200': (200, 64, 64)}[what]
  X, D, C, _ = _fc_problem(device, 47, b, n, s)
  if what == 'offset-view':
    flat = torch.zeros(C.numel() + 1, device=device)
    flat[1:] = C.reshape(-1)
    C = flat[1:].view(b, s)
    assert C.data_ptr() % 16 == 4
  forced = _gradient(X, D, C, 'b3', monkeypatch, 'f32').clone()
  assert torch.equal(forced, _gradient(X, D, C, 'f32', monkeypatch, 'f32'))
