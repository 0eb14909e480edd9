"""Every dictionary-update route on its gradient, against float64.

Each case names the route it takes; a Python mirror of the C dispatch asserts
it, so a dispatch change fails here instead of quietly moving coverage.  Per
case: grad_sum from the C entry point against the float64 gradient
(update_oracle.GRAD_GATES), the plugin's step D_after - D0 against the float64
step at a step size that moves D by a few percent (update_oracle.STEP_GATES;
tests/test_update_gates_host.py shows that each catches a 1e-4 gradient
error), and two runs bit for bit.  Measured errors:
profiles/precision_updates.txt."""
import ctypes

import numpy as np
import pytest
import torch

import helpers
import sc_oracle
import update_oracle as uo

pytestmark = pytest.mark.gpu

ceil_div = lambda a, b: -(-a // b)


def _report(name, route, **errors):
  print('%-34s %-18s %s' % (name, route, '  '.join(
      '%s %.2e' % kv for kv in sorted(errors.items()))))


def _gemm_prefers_small(m, n):
  """gemm_prefers_small (csrc/gemm_f32.h): 128 x 128 tiles."""
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  return ceil_div(m, 128) * ceil_div(n, 128) <= 8 or m * n / 16384. <= cus


# ------------------------------------------------------------ fully connected
def _fc_gradient_route(b, n, s):
  """vtc_fc_dict_gradient (csrc/dict_update.hip)."""
  return 'fc-small' if b <= 512 and _gemm_prefers_small(s, n) else (
      'fc-split-k')


def _fc_apply_route(dictionary, n):
  """Rows per block of vtc_fc_dict_apply: whole 128-byte lines per block,
  one block for a dictionary that does not start on a line."""
  if dictionary.data_ptr() % 128:
    return 'single-block'
  rows = 32
  while rows > 4 and (rows // 2) * n * 4 % 128 == 0:
    rows //= 2
  return 'rows%d' % rows


def _fc_problem(device, seed, b, n, s):
  rs = np.random.RandomState(seed)
  X = helpers.to_dev((0.1 * rs.randn(b, n)).astype(np.float32), device)
  D = helpers.to_dev(helpers.unit_rows(seed + 1, s, n), device)
  C = helpers.to_dev((0.05 * rs.randn(b, s) * (rs.rand(b, s) < 0.2)).astype(
      np.float32), device)
  h = helpers.to_dev((0.01 + 0.05 * rs.rand(s)).astype(np.float32), device)
  return X, D, C, h


def _fc_gradient(X, D, C):
  import vtc_hip
  lib = vtc_hip.load_library()
  b, n = X.shape
  s = D.shape[0]
  ws = vtc_hip.workspace(lib.vtc_fc_dict_gradient_workspace_bytes(b, n, s),
                         X.device)
  out = torch.empty(s, n, device=X.device)
  vtc_hip.check(lib.vtc_fc_dict_gradient(
      vtc_hip.ptr(X), vtc_hip.ptr(D), vtc_hip.ptr(C), vtc_hip.ptr(out), b, n,
      s, vtc_hip.ptr(ws), ws.numel(), vtc_hip.current_stream(X.device)),
      'vtc_fc_dict_gradient')
  return out


# (name, b, n, s, gradient route, apply route)
FC_CASES = [
    ('fc small ragged', 97, 15, 75, 'fc-small', 'rows32'),
    ('fc small example size', 512, 256, 1024, 'fc-small', 'rows4'),
    ('fc split-K ragged', 600, 18, 45, 'fc-split-k', 'rows16'),
    ('fc split-K b<=512 wide', 200, 1500, 3000, 'fc-split-k', 'rows8'),
    ('fc split-K large', 4096, 12, 1024, 'fc-split-k', 'rows8'),
]


@pytest.mark.parametrize('case', FC_CASES, ids=[c[0] for c in FC_CASES])
def test_fc_update_routes(device, case):
  """vtc_fc_dict_gradient on both routes, then both FC plugins, normalised
  and not."""
  from dict_update_rules.fully_connected import sc_steepest_descent
  from dict_update_rules.fully_connected import sc_cheap_quadratic_descent
  name, b, n, s, route, apply_route = case
  assert _fc_gradient_route(b, n, s) == route
  X, D0, C, h = _fc_problem(device, 100 + n, b, n, s)
  assert _fc_apply_route(D0, n) == apply_route
  grad = _fc_gradient(X, D0, C)
  assert torch.equal(grad, _fc_gradient(X, D0, C))
  ref_grad = uo.fc_gradient_sum(X, D0, C)
  grad_err = uo.rel(grad, ref_grad)
  step_errs = {}
  for rule, hess in (('steepest', None), ('cheapquad', h)):
    for normalize in (True, False):
      eta = uo.fc_stepsize(D0, ref_grad, b, hess)
      ref = uo.fc_apply(D0, ref_grad, b, eta, hess, normalize=normalize)
      assert uo.step_fraction(ref, D0) >= uo.MIN_STEP_FRACTION
      runs = []
      for _ in range(2):
        D = D0.clone()
        if hess is None:
          sc_steepest_descent.run(X, D, C, stepsize=eta,
                                  normalize_dictionary=normalize)
        else:
          sc_cheap_quadratic_descent.run(X, D, C, hess, stepsize=eta,
                                         normalize_dictionary=normalize)
        runs.append(D)
      assert torch.equal(runs[0], runs[1]), (rule, normalize)
      step_errs['%s%s' % (rule, '' if normalize else '-nonorm')] = (
          uo.step_error(runs[0], ref, D0))
  _report(name, route + '/' + apply_route, grad=grad_err, **step_errs)
  assert grad_err < uo.GRAD_GATES[route]
  for key, err in step_errs.items():
    assert err < uo.STEP_GATES['fc'], key


@pytest.mark.parametrize('n', [15, 18, 12, 256])
def test_fc_apply_unaligned_view(device, n):
  """vtc_fc_dict_apply on a contiguous view that does not start on a
  128-byte line takes the single-block branch: bit for bit the aligned
  result, the floats on either side untouched, and the step within the FC
  gate of float64.  n covers every rows-per-block choice of the aligned
  launch (32, 16, 8, 4)."""
  import vtc_hip
  lib = vtc_hip.load_library()
  s, b, k, tail = 37, 64, 5, 64
  X, D0, C, h = _fc_problem(device, 200 + n, b, n, s)
  grad = _fc_gradient(X, D0, C)
  rs = np.random.RandomState(n)
  P = helpers.to_dev(rs.randn(s, n).astype(np.float32), device)
  canary = 1234.5
  stream = vtc_hip.current_stream(device)
  for hess, pen, lam, normalize in ((None, None, 0.0, 1),
                                    (h, P, 0.05, 0)):
    ref_grad = grad.double()
    eta = uo.fc_stepsize(D0, ref_grad, b, hess, pen, lam)
    ref = uo.fc_apply(D0, ref_grad, b, eta, hess, pen, lam, normalize)
    outs = {}
    buf = torch.full((k + s * n + tail,), canary, device=device)
    view = buf[k:k + s * n].view(s, n)
    view.copy_(D0)
    aligned = D0.clone()
    for D in (aligned, view):
      route = _fc_apply_route(D, n)
      vtc_hip.check(lib.vtc_fc_dict_apply(
          vtc_hip.ptr(D), vtc_hip.ptr(grad), vtc_hip.ptr(hess),
          vtc_hip.ptr(pen), lam, b, eta, uo.LOWEST_CODE_VAL, normalize, s, n,
          stream), 'vtc_fc_dict_apply')
      outs[route] = D
    assert sorted(outs) == sorted(['single-block', _fc_apply_route(D0, n)])
    err = uo.step_error(aligned, ref, D0)
    _report('fc apply n=%d%s' % (n, '' if hess is None else ' hess+pen'),
            '/'.join(sorted(outs)), step=err)
    assert torch.equal(aligned, view)
    assert bool((buf[:k] == canary).all()) and bool(
        (buf[k + s * n:] == canary).all())
    assert err < uo.STEP_GATES['fc']


# ---------------------------------------------------------------- subspace
def _alignment_route(m, n):
  from dict_update_rules.fully_connected import (
      subspace_sc_cheap_quadratic_descent as plugin)
  if not plugin.alignment_fits_device(m, n):
    return 'float64-fallback'
  return 'lds-dynamic' if (m * n + m * m + m) * 4 > 64 * 1024 else 'lds'


def _subspace_problem(device, seed, sizes, n, normalized, overlap=False):
  """Groups of the given sizes; each member is +-(a shared direction) plus
  noise, so that every within-group |cos| is well above 1e-3 and float32 and
  float64 agree on its sign."""
  rs = np.random.RandomState(seed)
  rows, groups = [], []
  for size in sizes:
    u = rs.randn(n)
    u /= np.linalg.norm(u)
    sign = np.where(rs.rand(size) < 0.5, -1.0, 1.0)
    block = sign[:, None] * u[None, :] + rs.randn(size, n) / np.sqrt(n)
    groups.append(list(range(len(rows), len(rows) + size)))
    rows.extend(block)
  d = np.array(rows)
  d /= np.linalg.norm(d, axis=1, keepdims=True)
  if not normalized:
    d *= rs.uniform(0.5, 2.0, (len(d), 1))
  if overlap:   # atoms in two groups: the CSR sum over an atom's slots
    groups.append([groups[0][0], groups[-1][-1], groups[1][0]])
  d = d.astype(np.float32)
  for g in groups:
    rows64 = d[g].astype(np.float64)
    nrm = np.linalg.norm(rows64, axis=1)
    cos = rows64 @ rows64.T / np.outer(nrm, nrm)
    assert np.abs(cos).min() >= 1e-3
  s = len(d)
  b = 96
  X = helpers.to_dev((0.1 * rs.randn(b, n)).astype(np.float32), device)
  C = helpers.to_dev((0.05 * rs.randn(b, s) * (rs.rand(b, s) < 0.2)).astype(
      np.float32), device)
  h = helpers.to_dev((0.01 + 0.05 * rs.rand(s)).astype(np.float32), device)
  return X, helpers.to_dev(d, device), C, h, groups


def _alignment_gradient(D, groups, normalized):
  import vtc_hip
  from vtc_hip import groups as group_tables
  lib = vtc_hip.load_library()
  s, n = D.shape
  t = group_tables.tables_for(groups, s, D.device)
  ws = vtc_hip.workspace(
      lib.vtc_subspace_alignment_gradient_workspace_bytes(t.slots, n),
      D.device)
  out = torch.empty(s, n, device=D.device)
  vtc_hip.check(lib.vtc_subspace_alignment_gradient(
      vtc_hip.ptr(D), vtc_hip.ptr(t.index), vtc_hip.ptr(t.valid),
      vtc_hip.ptr(t.atom_ptr), vtc_hip.ptr(t.atom_slots), vtc_hip.ptr(out),
      s, n, t.num_groups, t.m, 1 if normalized else 0, vtc_hip.ptr(ws),
      ws.numel(), vtc_hip.current_stream(D.device)),
      'vtc_subspace_alignment_gradient')
  return out


# (name, group sizes, n, overlapping groups, route)
SUBSPACE_CASES = [
    ('ragged groups up to 7', [1, 5, 2, 7, 6, 3, 5, 4], 60, True, 'lds'),
    ('groups of 32, n=64', [32] * 8, 64, False, 'lds'),
    ('groups of 32, n=576', [32] * 4, 576, False, 'lds-dynamic'),
    ('groups of 64, n=256', [64] * 4, 256, False, 'lds-dynamic'),
    ('groups of 128, n=64', [128, 128], 64, True, 'lds-dynamic'),
    ('groups of 64, n=640', [64, 64], 640, False, 'float64-fallback'),
]


@pytest.mark.parametrize('case', SUBSPACE_CASES,
                         ids=[c[0] for c in SUBSPACE_CASES])
def test_subspace_update_routes(device, case):
  """vtc_subspace_alignment_gradient against the summed float64
  alignment_gradients, then subspace_sc_cheap_quadratic_descent with
  penalty 0 and 0.05, normalised and not, against float64."""
  import warnings
  from dict_update_rules.fully_connected import (
      subspace_sc_cheap_quadratic_descent as plugin)
  name, sizes, n, overlap, route = case
  m = max(sizes)
  assert _alignment_route(m, n) == route
  errs = {}
  for normalized in (True, False):
    tag = '' if normalized else '-nonorm'
    X, D0, C, h, groups = _subspace_problem(device, 300 + m + n, sizes, n,
                                            normalized, overlap)
    b = X.shape[0]
    ref_pen = uo.alignment_gradient_sum(D0, groups, normalized)
    if route == 'float64-fallback':
      with pytest.raises(NotImplementedError):
        _alignment_gradient(D0, groups, normalized)
    else:
      pen = _alignment_gradient(D0, groups, normalized)
      assert torch.equal(pen, _alignment_gradient(D0, groups, normalized))
      errs['align' + tag] = uo.rel(pen, ref_pen)
    ref_grad = uo.fc_gradient_sum(X, D0, C)
    for lam in (0.0, 0.05):
      eta = uo.fc_stepsize(D0, ref_grad, b, h, ref_pen, lam)
      ref = uo.fc_apply(D0, ref_grad, b, eta, h, ref_pen, lam, normalized)
      assert uo.step_fraction(ref, D0) >= uo.MIN_STEP_FRACTION
      runs = []
      for _ in range(2):
        D = D0.clone()
        with warnings.catch_warnings(record=True) as caught:
          warnings.simplefilter('always')
          plugin.run(X, D, C, groups, h, lam, stepsize=eta,
                     normalize_dictionary=normalized)
        fell_back = any('float64 torch' in str(w.message) for w in caught)
        assert fell_back == (route == 'float64-fallback' and lam != 0)
        runs.append(D)
      assert torch.equal(runs[0], runs[1])
      errs['step-pen%g%s' % (lam, tag)] = uo.step_error(runs[0], ref, D0)
  _report(name, route, **errs)
  for key, err in errs.items():
    gate = (uo.GRAD_GATES['alignment'] if key.startswith('align') else
            uo.STEP_GATES['subspace'])
    assert err < gate, key


# ----------------------------------------------------------- convolutional
def _conv_gradient_route(geom, precision):
  """vtc_conv_dict_gradient (csrc/conv.hip) for geometries of the C struct,
  mirroring patch_geometry / patch_gradient_small (conv_patch.h) and
  unit_geometry (conv_unit.h); the matrix-core route is taken on request."""
  if precision != 'f32':
    return 'conv-bf16x3'
  cover = ceil_div(geom.kh, geom.stride_v) * ceil_div(geom.kw, geom.stride_h)
  taps = geom.c * geom.kh * geom.kw
  ch = (geom.h - geom.kh) // geom.stride_v + 1
  cw = (geom.w - geom.kw) // geom.stride_h + 1
  if ((geom.stride_v > 1 or geom.stride_h > 1) and cover <= 16 and
      taps <= 8192 and geom.b <= 65535 and geom.b * ch * cw < (1 << 31)):
    small = geom.b <= 16 and _gemm_prefers_small(geom.s, taps)
    return 'conv-patch-small' if small else 'conv-patch'
  if (geom.stride_v == 1 and geom.stride_h == 1 and geom.kh == geom.kw and
      geom.kh in (5, 8, 11, 16)):
    return 'conv-unit'
  return 'conv-direct'


def _plugin_precision(geom):
  """What the conv plugins run under precision 'auto'
  (dict_update_rules/convolutional/_common.py)."""
  import vtc_hip
  lib = vtc_hip.load_library()
  ok = geom.s >= 32 and lib.vtc_conv_x3_supported(ctypes.byref(geom))
  return 'bf16x3' if ok else 'f32'


def _x3_structural(geom):
  """The shape part of cx_plan (conv_x3.h); the rest is its LDS budget."""
  return (1 <= geom.c <= 8 and geom.stride_v == 1 and geom.stride_h == 1 and
          geom.kh == geom.kw and geom.kh in (5, 8, 11, 16))


def _conv_problem(device, seed, c, kh, kw, stride, s, b, height, width):
  rs = np.random.RandomState(seed)
  lead_v, trail_v = sc_oracle.conv_padding_amount(height, kh, stride[0])
  lead_h, trail_h = sc_oracle.conv_padding_amount(width, kw, stride[1])
  x = np.zeros((b, c, height + lead_v + trail_v, width + lead_h + trail_h),
               np.float32)
  x[:, :, lead_v:lead_v + height, lead_h:lead_h + width] = 0.5 * rs.randn(
      b, c, height, width)
  d = rs.randn(s, c, kh, kw).astype(np.float32)
  d /= np.sqrt((d.astype(np.float64) ** 2).sum(axis=(1, 2, 3)))[
      :, None, None, None].astype(np.float32)
  ch = sc_oracle.conv_code_dim(x.shape[2], kh, stride[0])
  cw = sc_oracle.conv_code_dim(x.shape[3], kw, stride[1])
  codes = (0.05 * rs.randn(b, s, ch, cw) *
           (rs.rand(b, s, ch, cw) < 0.2)).astype(np.float32)
  h = (0.01 + 0.05 * rs.rand(s)).astype(np.float32)
  pad = ((lead_v, trail_v), (lead_h, trail_h))
  return (helpers.to_dev(x, device), helpers.to_dev(d, device),
          helpers.to_dev(codes, device), helpers.to_dev(h, device), pad)


def _conv_gradient(X, D, C, geom, precision):
  import vtc_hip
  lib = vtc_hip.load_library()
  ws = vtc_hip.workspace(
      lib.vtc_conv_dict_gradient_workspace_bytes(ctypes.byref(geom)),
      X.device)
  out = torch.empty_like(D)
  vtc_hip.check(lib.vtc_conv_dict_gradient(
      vtc_hip.ptr(X), vtc_hip.ptr(D), vtc_hip.ptr(C), vtc_hip.ptr(out),
      ctypes.byref(geom), vtc_hip.PRECISIONS[precision], vtc_hip.ptr(ws),
      ws.numel(), vtc_hip.current_stream(X.device)), 'vtc_conv_dict_gradient')
  return out


def _largest_x3_channels(k):
  """The largest channel count cx_plan accepts for k x k kernels (at the
  geometry of the case below)."""
  import vtc_hip
  lib = vtc_hip.load_library()
  best = 0
  for c in range(1, 9):
    g = vtc_hip.ConvGeometry()
    g.b, g.c, g.h, g.w, g.s = 2, c, 30 + 2 * (k - 1), 40 + 2 * (k - 1), 32
    g.kh = g.kw = k
    g.stride_v = g.stride_h = 1
    if lib.vtc_conv_x3_supported(ctypes.byref(g)):
      best = c
  return best


# (name, c, kh, kw, stride, s, b, height, width, precision, route)
CONV_CASES = [
    ('bf16x3 c=2 k=5', 2, 5, 5, (1, 1), 40, 3, 41, 70, 'bf16x3',
     'conv-bf16x3'),
    ('bf16x3 c=3 k=8', 3, 8, 8, (1, 1), 33, 2, 33, 50, 'bf16x3',
     'conv-bf16x3'),
    ('bf16x3 c=4 k=11', 4, 11, 11, (1, 1), 64, 2, 37, 44, 'bf16x3',
     'conv-bf16x3'),
    ('bf16x3 largest c k=5', 'max', 5, 5, (1, 1), 32, 2, 30, 40, 'bf16x3',
     'conv-bf16x3'),
    ('bf16x3 largest c k=16', 'max', 16, 16, (1, 1), 32, 2, 30, 40,
     'bf16x3', 'conv-bf16x3'),
    ('bf16x3 large c=2 k=11', 2, 11, 11, (1, 1), 128, 8, 128, 128, 'bf16x3',
     'conv-bf16x3'),
    ('patch-small ragged', 2, 6, 6, (2, 2), 9, 3, 31, 29, 'f32',
     'conv-patch-small'),
    ('patch-small large', 1, 8, 8, (4, 4), 32, 16, 256, 256, 'f32',
     'conv-patch-small'),
    ('patch b=19 ragged', 1, 6, 9, (3, 3), 11, 19, 40, 35, 'f32',
     'conv-patch'),
    ('patch b=64 large', 1, 8, 8, (4, 4), 64, 64, 128, 128, 'f32',
     'conv-patch'),
    ('patch wide bank', 64, 8, 8, (2, 2), 1040, 2, 26, 26, 'f32',
     'conv-patch'),
    ('unit ragged k=11', 1, 11, 11, (1, 1), 9, 3, 37, 50, 'f32', 'conv-unit'),
    ('unit c=2 k=8', 2, 8, 8, (1, 1), 40, 2, 33, 29, 'f32', 'conv-unit'),
    ('unit large k=16', 1, 16, 16, (1, 1), 64, 8, 128, 128, 'f32',
     'conv-unit'),
    ('direct non-square', 2, 5, 7, (1, 1), 13, 3, 30, 41, 'f32',
     'conv-direct'),
    ('direct k=7 c=3', 3, 7, 7, (1, 1), 34, 2, 27, 31, 'f32', 'conv-direct'),
    ('direct k=16 stride 2 large', 1, 16, 16, (2, 2), 32, 32, 128, 128, 'f32',
     'conv-direct'),
]


@pytest.mark.parametrize('case', CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_update_routes(device, case):
  """vtc_conv_dict_gradient on every route, then both conv plugins at
  eta = 0.03 (the global rescale moves D by 3 %)."""
  import vtc_hip
  from utils import convolutions
  from dict_update_rules.convolutional import sc_steepest_descent
  from dict_update_rules.convolutional import sc_cheap_quadratic_descent
  name, c, kh, kw, stride, s, b, height, width, precision, route = case
  if c == 'max':
    c = _largest_x3_channels(kh)
    assert c >= 1
  X, D0, C, h, pad = _conv_problem(device, 500 + c * kh + s, c, kh, kw,
                                   stride, s, b, height, width)
  geom = convolutions.geometry(X, D0, stride, pad)
  assert _conv_gradient_route(geom, precision) == route
  lib = vtc_hip.load_library()
  x3 = bool(lib.vtc_conv_x3_supported(ctypes.byref(geom)))
  if route == 'conv-bf16x3':
    assert x3 and _x3_structural(geom)
    if case[1] == 'max' and c < 8:
      geom.c = c + 1
      assert not lib.vtc_conv_x3_supported(ctypes.byref(geom))
      geom.c = c
  grad = _conv_gradient(X, D0, C, geom, precision)
  assert torch.equal(grad, _conv_gradient(X, D0, C, geom, precision))
  ref_grad = uo.conv_gradient_sum(X, D0, C, stride, pad)
  grad_err = uo.rel(grad, ref_grad)
  step_errs = {}
  saved = vtc_hip.get_default_precision()
  # 'auto' where it picks the route under test; exact f32 asked for otherwise
  plugin_mode = 'auto' if (route == 'conv-bf16x3' or
                           _plugin_precision(geom) == 'f32') else 'f32'
  try:
    vtc_hip.set_default_precision(plugin_mode)
    for rule, hess in (('steepest', None), ('cheapquad', h)):
      ref = uo.conv_apply(D0, ref_grad, b, uo.STEP_FRACTION, hess)
      assert uo.step_fraction(ref, D0) >= uo.MIN_STEP_FRACTION
      runs = []
      for _ in range(2):
        D = D0.clone()
        if hess is None:
          sc_steepest_descent.run(X, D, C, stride, pad,
                                  stepsize=uo.STEP_FRACTION)
        else:
          sc_cheap_quadratic_descent.run(X, D, C, hess, stride, pad,
                                         stepsize=uo.STEP_FRACTION)
        runs.append(D)
      assert torch.equal(runs[0], runs[1]), rule
      step_errs[rule] = uo.step_error(runs[0], ref, D0)
  finally:
    vtc_hip.set_default_precision(saved)
  _report('%s (c=%d)' % (name, c), route, grad=grad_err, **step_errs)
  assert grad_err < uo.GRAD_GATES[route]
  step_gate = uo.STEP_GATES['conv-bf16x3' if route == 'conv-bf16x3' else
                            'conv-f32']
  for rule, err in step_errs.items():
    assert err < step_gate, rule


@pytest.mark.parametrize('b,s,ch,cw', [(5, 13, 17, 23), (64, 100, 57, 57)])
def test_conv_code_energy(device, b, s, ch, cw):
  """vtc_code_energy over code maps (positions > 1) and vtc_hessian_ema,
  against float64 (training/sparse_coding.py:160-161)."""
  import vtc_hip
  lib = vtc_hip.load_library()
  rs = np.random.RandomState(b + s)
  codes = (rs.randn(b, s, ch, cw) * (rs.rand(b, s, ch, cw) < 0.3)).astype(
      np.float32)
  h0 = (0.01 + 0.05 * rs.rand(s)).astype(np.float32)
  C, h = helpers.to_dev(codes, device), helpers.to_dev(h0, device)
  positions = ch * cw
  stream = vtc_hip.current_stream(device)
  ws = vtc_hip.workspace(lib.vtc_code_energy_workspace_bytes(b, s, positions),
                         device)
  energies = []
  for _ in range(2):
    energy = torch.empty(s, device=device)
    vtc_hip.check(lib.vtc_code_energy(
        vtc_hip.ptr(C), b, s, positions, vtc_hip.ptr(energy), vtc_hip.ptr(ws),
        ws.numel(), stream), 'vtc_code_energy')
    energies.append(energy)
  assert torch.equal(energies[0], energies[1])
  vtc_hip.check(lib.vtc_hessian_ema(vtc_hip.ptr(h), vtc_hip.ptr(energies[0]),
                                    b, s, stream), 'vtc_hessian_ema')
  c64 = torch.from_numpy(codes).double()
  ref_energy = (c64 ** 2).sum(dim=(0, 2, 3))
  ref_h = sc_oracle.hessian_diag_ema_(torch.from_numpy(h0).double(), c64)
  e_err = uo.rel(energies[0].cpu(), ref_energy)
  h_err = uo.rel(h.cpu(), ref_h)
  _report('code energy b=%d s=%d %dx%d' % (b, s, ch, cw), 'maps',
          energy=e_err, ema=h_err)
  assert e_err < uo.ENERGY_GATE and h_err < uo.ENERGY_GATE
