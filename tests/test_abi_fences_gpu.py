"""Every C ABI entry point behind guard bands (tests/fences.py).

include/vtc_hip.h promises that a call writes its outputs and its workspace
and nothing else, with the workspace sized by the matching query.  The rest of
the suite reaches the library through the plugins, whose scratch comes from
torch's caching allocator: that rounds every request up, so an overrun of a
few KiB lands in slack and no value test sees it.  Here each case calls the
raw ctypes function twice:

  plain   inputs in ordinary tensors, zero-filled outputs, a zero-filled
          workspace of more than twice the queried size          -> `want`
  fenced  inputs, outputs and workspace each inside [guard | payload | guard]
          arenas, outputs and workspace pre-filled with 0xFF (NaN), the
          workspace of EXACTLY the queried size                   -> `got`

and asserts: status VTC_OK, every guard intact (inputs included), inputs
bitwise unchanged, outputs finite where the contract writes them, and
torch.equal(got, want) -- the library documents fixed summation orders, so a
difference means the result depends on what the scratch held or where it lay.
One truth check per case on `want` (float64 reference) keeps two identically
wrong calls from passing.

Workspace edges.  Where one route stands behind the query, a call with one
byte less must return VTC_ERR_WORKSPACE and touch nothing.  Where the query is
the largest need of several routes (vtc_fc_ista_fista in the split
precisions, vtc_subspace_ista_fista, the exact-f32 on-chip kernels behind the
tiled query), the case restates the size its own route carves, checks the
query against those sizes, runs a third fenced call in exactly that many
bytes -- same bits again -- and asks for the refusal at one byte less than
THAT, by the size check of that route (the head of vtc_last_error names it).
This is also the evidence that the call took the route the case is there for.
Where the header allows no workspace the fenced call passes (NULL, 0).

Bounds.  Inference: tests/helpers.py tolerances for the route and horizon.
Updates: REL_TOL_DICT.  Reductions: the forward-error bound of a length-K
float32 summation, K * 2^-24 * sum |terms| from the float64 reference, plus
K * 2^-149 where terms can underflow (a squared denormal is an exact 0 in
float32).  Data movement and counts are exact.  Entry points whose accuracy an
older test already gates (eigen-solvers, FFT whitening, float64 moments) keep
that test's figure.

CASES is imported as data by tests/test_abi_fences_host.py, which fails when
an entry point of the header has no row here.
"""
import ctypes

import numpy as np
import pytest
import torch

import fences
import helpers
import sc_oracle
import update_oracle

pytestmark = pytest.mark.gpu

OK, ERR_WORKSPACE = 0, 3
ISTA, FISTA = 0, 1
SOFT, SOFT_NONNEG, HARD, HARD_NONNEG = range(4)
F32, BF16X3, BF16, F16X3 = range(4)
PREC_NAME = {F32: 'f32', BF16X3: 'bf16x3', BF16: 'bf16', F16X3: 'f16x3'}
U24 = 2.0 ** -24        # unit roundoff of float32
TINY = 2.0 ** -149      # smallest float32 subnormal
REL_TOL_BF16 = 5e-2     # tests/test_fc_fused_gpu.py: single bf16 product
FLIP_BF16X3 = 5e-6      # tests/test_fc_fused_gpu.py SPLIT['bf16x3']


def _lib():
  import vtc_hip
  return vtc_hip.load_library()


def _ceil(a, b):
  return -(-a // b)


def _x3_want_slices(M, N, K):
  """gemm_x3_want_slices (csrc/gemm_x3.h)."""
  want = min(_ceil(512, _ceil(M, 128) * _ceil(N, 128)), _ceil(K, 256), 16)
  want = max(want, 1)
  chunk = max(_ceil(_ceil(K, want), 32) * 32, 32)
  return _ceil(K, chunk)


class Spec(object):
  """One call: numpy inputs (None = NULL), output shapes (None = NULL), the
  names of inputs the call updates in place, and closures.

  ws_bytes is what the *_workspace_bytes() query answers (0: the entry point
  has no workspace, or the header allows (NULL, 0) and the case passes that).
  need is what the route the case takes carves for itself: the query where
  one route stands behind it (the default with tight=True), less where the
  query is the largest need of several routes.  A route with a need is
  called with need - 1 bytes and must refuse; gate is the head of the error
  text of the size check that has to answer, which names the route."""

  def __init__(self, inputs, outputs, call, truth, ws_bytes=0, tight=False,
               need=None, gate=None, inout=(), route=None):
    self.inputs, self.outputs = inputs, outputs
    self.call, self.truth = call, truth
    self.ws_bytes = int(ws_bytes)
    self.need = self.ws_bytes if (tight and need is None) else need
    self.gate = gate
    self.inout = tuple(inout)
    self.route = route
    self.host = {}                  # host-side results (iters_run)


class Case(object):
  def __init__(self, entry, name, branch, make):
    self.entry, self.name, self.branch, self.make = entry, name, branch, make
    self.id = '%s-%s' % (entry[4:], name)


CASES = []


def case(entry, name, branch):
  def deco(make):
    CASES.append(Case(entry, name, branch, make))
    return make
  return deco


def _p(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _np(t):
  return t.detach().cpu().numpy()


def _geom(d):
  import vtc_hip
  return vtc_hip.ConvGeometry(**d)


# --------------------------------------------------------------------- runner
def run_case(device, c):
  import vtc_hip
  lib = _lib()
  spec = c.make(lib)
  if spec.route is not None:
    spec.route(lib)
  stream = vtc_hip.current_stream(device)
  what = c.id

  def tensors(fenced_arena):
    t, f = {}, {}
    for k, v in spec.inputs.items():
      if v is None:
        t[k] = None
      elif fenced_arena:
        t[k], f[k] = fences.fenced_copy(v, device)
      else:
        t[k] = helpers.to_dev(v, device).clone()
    for k, shape_dtype in spec.outputs.items():
      if shape_dtype is None:
        t[k] = None
        continue
      shape, dtype = shape_dtype
      dtype = torch.from_numpy(np.zeros(1, dtype)).dtype
      if fenced_arena:
        t[k], f[k] = fences.fenced(shape, dtype, device)
      else:
        t[k] = torch.zeros(shape, dtype=dtype, device=device)
    return t, f

  def results(t):
    names = [k for k, v in spec.outputs.items() if v is not None]
    return {k: t[k] for k in names + list(spec.inout)}

  # plain call
  t0, _ = tensors(False)
  ws0 = torch.zeros(2 * spec.ws_bytes + (1 << 20), dtype=torch.uint8,
                    device=device)
  rc = spec.call(lib, {k: _p(v) for k, v in t0.items()}, _p(ws0),
                 ws0.numel(), stream)
  torch.cuda.synchronize(device)
  assert rc == OK, '%s plain: %s' % (what, lib.vtc_last_error())
  want = results(t0)
  host_want = dict(spec.host)

  def fenced_call(nbytes, label):
    """The call on fenced inputs, 0xFF-filled fenced outputs and a 0xFF-filled
    fenced workspace of exactly nbytes (0: NULL)."""
    t, f = tensors(True)
    ws_ptr = ctypes.c_void_p(0)
    if nbytes > 0:
      ws, f['workspace'] = fences.fenced_workspace(nbytes, device)
      ws_ptr = _p(ws)
    rc = spec.call(lib, {k: _p(v) for k, v in t.items()}, ws_ptr, nbytes,
                   stream)
    torch.cuda.synchronize(device)
    for k, fence in f.items():
      fence.assert_intact('%s (%s): %s' % (what, label, k))
    return rc, t, f

  def inputs_unchanged(t, label, names):
    for k in names:
      v = spec.inputs[k]
      if v is not None:
        assert torch.equal(t[k].cpu(), torch.from_numpy(np.ascontiguousarray(
            v)).reshape(t[k].shape)), (
                '%s (%s): input %s was modified' % (what, label, k))

  def same_as_plain(t, f, label):
    inputs_unchanged(t, label, [k for k in spec.inputs
                                if k not in spec.inout])
    for k, v in results(t).items():
      if v.dtype.is_floating_point:
        f[k].assert_written('%s (%s): %s' % (what, label, k))
      assert torch.equal(v, want[k]), (
          '%s (%s): %s differs from the plain call in %d elements'
          % (what, label, k, int((v != want[k]).sum())))
    assert spec.host == host_want, what

  # fenced call, poisoned workspace of exactly the queried size
  rc, t1, f1 = fenced_call(spec.ws_bytes, 'queried size')
  assert rc == OK, '%s fenced: %s' % (what, lib.vtc_last_error())
  same_as_plain(t1, f1, 'queried size')

  # truth, on the plain call's result
  worst = 0.0
  for label, err, bound in spec.truth({k: _np(v) for k, v in want.items()},
                                      dict(spec.inputs)):
    print('abi_fence %-52s %-14s err %.3e bound %.3e' % (what, label, err,
                                                          bound))
    assert err <= bound, '%s %s: %.3e > %.3e' % (what, label, err, bound)
    worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else
                                                      float('inf')))
  print('abi_fence_row %-52s ws %12d need %12s worst %.3f  [%s]' % (
      what, spec.ws_bytes, '-' if spec.need is None else spec.need, worst,
      c.branch))

  # workspace edges
  if spec.need is None:
    return
  assert 0 <= spec.need <= spec.ws_bytes, what
  if spec.need < spec.ws_bytes:
    # the query is the largest need of several routes: this route must also
    # run, and give the same bits, in exactly what it carves for itself
    rc, t3, f3 = fenced_call(spec.need, "the route's own size")
    assert rc == OK, '%s at its own size: %s' % (what, lib.vtc_last_error())
    same_as_plain(t3, f3, "the route's own size")
  if spec.need > 0:
    rc, t2, f2 = fenced_call(spec.need - 1, 'one byte short')
    assert rc == ERR_WORKSPACE, '%s: one byte short gave %d' % (what, rc)
    text = lib.vtc_last_error().decode()
    if spec.gate is not None:
      assert text.startswith(spec.gate), (
          '%s: refused by "%s", not by the size check of its route ("%s")'
          % (what, text, spec.gate))
    inputs_unchanged(t2, 'one byte short', list(spec.inputs))
    for k, fence in f2.items():
      if k in spec.outputs or k == 'workspace':
        fence.assert_untouched('%s (one byte short): %s' % (what, k))


# ------------------------------------------------------------ shared checkers
def _codes_truth(ours, ref, prec, label):
  if prec == BF16:
    err = helpers.rel_err(ours, ref)
    assert np.isfinite(ours).all()
    return [(label, err, REL_TOL_BF16)]
  tol = helpers.REL_TOL_BF16X3 if prec == BF16X3 else helpers.REL_TOL_SHORT
  flip = FLIP_BF16X3 if prec == BF16X3 else helpers.NEAR_THRESHOLD
  err, _ = helpers.assert_codes_match(ours, ref, tol, label,
                                      max_flip_mag=flip)
  return [(label, err, tol)]


def _sum_bound(terms64, axis=-1):
  """K * 2^-24 * sum |terms| (+ K * 2^-149 for underflow) per output."""
  k = terms64.shape[axis]
  return k * (U24 * np.abs(terms64).sum(axis=axis) + TINY)


def _elementwise(label, ours, ref, bound):
  """Worst err / bound over the elements, reported against 1."""
  ours = np.asarray(ours, np.float64)
  assert np.isfinite(ours).all(), label
  bound = np.broadcast_to(np.asarray(bound, np.float64), ours.shape)
  err = np.abs(ours - ref)
  if (bound == 0).any():
    assert (err[bound == 0] == 0).all(), label
  ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0.0)
  return (label, float(ratio.max()) if ratio.size else 0.0, 1.0)


def _exact(label, ours, ref):
  same = np.array_equal(np.asarray(ours), np.asarray(ref))
  return (label, 0.0 if same else 1.0, 0.0)


def _sparse_codes(rs, shape, density=0.1, scale=0.05):
  c = scale * rs.randn(*shape) * (rs.rand(*shape) < density)
  return c.astype(np.float32)


# ------------------------------------------------- fully-connected inference
def _fc(name, branch, n, s, b, prec, variant=FISTA, warm=False, eps=-1.0,
        dev=False, thr=SOFT, iters=12, route=None):
  entry = 'vtc_fc_ista_fista_dev' if dev else 'vtc_fc_ista_fista'

  @case(entry, name, branch)
  def make(lib):
    rs = np.random.RandomState(n * 7 + s + b)
    X = helpers.gaussian_patches(n + s + b, b, n)
    D = helpers.unit_rows(n * 3 + s, s, n)
    eta = float(sc_oracle.fc_stepsize(torch.from_numpy(D).double()))
    lam = 0.02
    inputs = {'images': X, 'dictionary': D,
              'initial': _sparse_codes(rs, (b, s)) if warm else None}
    if dev:
      inputs['eta'] = np.array([eta], np.float32)
      eta = float(inputs['eta'][0])
    eta = float(np.float32(eta))
    need = lib.vtc_fc_ista_fista_workspace_bytes(b, n, s, prec)

    def call(lib, p, ws, wsb, st):
      done = ctypes.c_int(-1)
      if dev:
        rc = lib.vtc_fc_ista_fista_dev(
            p['images'], p['dictionary'], p['initial'], p['codes'], b, n, s,
            p['eta'], lam, iters, variant, thr, eps, prec, ws, wsb,
            ctypes.byref(done), st)
      else:
        rc = lib.vtc_fc_ista_fista(
            p['images'], p['dictionary'], p['initial'], p['codes'], b, n, s,
            eta, lam, iters, variant, thr, eps, prec, ws, wsb,
            ctypes.byref(done), st)
      spec.host['iters'] = done.value
      return rc

    def truth(want, inp):
      r = min(b, 64)
      assert spec.host['iters'] == iters   # eps = 0 never fires
      init = (torch.from_numpy(inp['initial'][:r]).double()
              if warm else None)
      ref = sc_oracle.fc_ista_fista(
          torch.from_numpy(X[:r]).double(), torch.from_numpy(D).double(), lam,
          iters, variant='fista' if variant == FISTA else 'ista',
          initial_codes=init,
          early_stopping_epsilon=None if eps < 0 else float(eps),
          nonnegative_only=thr in (SOFT_NONNEG, HARD_NONNEG),
          hard_threshold=thr in (HARD, HARD_NONNEG), stepsize=eta)
      return _codes_truth(want['codes'][:r], ref.numpy(), prec, 'codes')

    route_need, gate = _fc_route(lib, route, b, n, s, prec, need)
    spec = Spec(inputs, {'codes': ((b, s), np.float32)}, call, truth,
                ws_bytes=need, need=route_need, gate=gate)
    return spec
  return make


def _au(nbytes):
  return _ceil(nbytes, 256) * 256      # align_up(., 256) of csrc/common.h


X3_STATE_BYTES = _au(4 * (64 + 4 * 32 * 32))   # kX3StateWords, kSubStateWords


def _tiled_need(b, n, s):
  """generic_workspace_bytes (csrc/fc_inference.hip) and, term for term,
  subspace_ws_bytes (csrc/subspace.hip)."""
  return (3 * _au(4 * b * s) + _au(4 * b * n) + _au(4 * s * n) +
          _au(4 * _x3_want_slices(b, n, s) * b * n) + 256 + X3_STATE_BYTES)


def _fused_need(s, prec):
  """fused_workspace_bytes (csrc/fc_fused.hip): hi (and lo) packs of D, D^T."""
  return (1 if prec == BF16 else 2) * 2 * _au(s * 256 * 2) + 256


def _stream_need(b, slots):
  """stream_workspace_bytes (csrc/fused_stream.hip)."""
  return (2 * _au(_ceil(b, 32) * 32 * slots * 4) +
          2 * _au(2 * slots * 256 * 2) + _au(4 * b) + 256)


def _chip16_need(n, s):
  return _au(4 * s * n) + 256        # chip16_workspace_bytes


FC_GATES = {'chip16': 'on-chip 12x12 kernel: workspace too small',
            'fused': 'fused FISTA: workspace too small',
            'stream': 'streamed fused FISTA: workspace too small',
            'tiled': 'vtc_fc_ista_fista: workspace too small'}


def _fc_route(lib, route, b, n, s, prec, query):
  """(what the route carves, head of its size check's error text), after
  checking the query against the sizes of the routes it is the largest of
  (vtc_fc_ista_fista_workspace_bytes).  The runner then shows that the call
  runs in exactly that much and that one byte less is refused by THAT size
  check: a call dispatched elsewhere is refused by another check, or not at
  all."""
  tiled = _tiled_need(b, n, s)
  assert tiled == lib.vtc_fc_ista_fista_workspace_bytes(b, n, s, F32)
  fused_shape = n == 256 and s in (256, 512, 1024)
  stream_shape = n == 256 and s % 256 == 0 and s <= 16384
  fused = _fused_need(s, prec) if fused_shape else 256
  stream = _stream_need(b, s) if stream_shape else 0
  if prec == F32:
    assert query == tiled
  elif prec == BF16:
    assert query == fused
  else:
    assert query == max(fused, tiled, stream)
  if route == 'small':
    assert prec == F32
    return 0, None         # run_small takes no workspace: (NULL, 0) must do
  need = {'chip16': _chip16_need(n, s), 'fused': fused, 'stream': stream,
          'tiled': tiled}[route]
  assert 256 < need <= query
  return need, FC_GATES[route]


BATCHES = (1, 31, 33, 100)
FUSED_OPTIONS = {256: ('2 phases, warm', dict(warm=True)),
                 512: ('4 phases', dict()),
                 1024: ('8 phases, ISTA', dict(variant=ISTA))}
for _b in BATCHES:
  for _dev in (False, True):
    _d = 'dev-' if _dev else ''
    _fc('%sfc_small-s64-b%d' % (_d, _b), 'run_small (no workspace used)', 64,
        64, _b, F32, variant=ISTA, dev=_dev, route='small')
    _fc('%schip16-144x576-b%d' % (_d, _b), 'run_chip16 packed dictionary',
        144, 576, _b, F32, dev=_dev, route='chip16')
    _fc('%sfused-s512-f16x3-b%d' % (_d, _b), 'run_fused 4 phases', 256, 512,
        _b, F16X3, dev=_dev, route='fused')
    _fc('%sstream-s1280-f16x3-b%d' % (_d, _b), 'run_stream state slabs', 256,
        1280, _b, F16X3, dev=_dev, route='stream')
    _fc('%stiled-f32-100x200-b%d' % (_d, _b), 'run_generic f32, ragged tiles',
        100, 200, _b, F32, dev=_dev, route='tiled')
  _fc('fc_small-s192-b%d' % _b, 'run_small, FISTA warm', 64, 192, _b, F32,
      warm=True, route='small')
  _fc('chip16-64x256-b%d' % _b, 'run_chip16, ISTA warm', 64, 256, _b, F32,
      variant=ISTA, warm=True, route='chip16')
  for _s in (256, 512, 1024):
    for _prec in (F16X3, BF16X3, BF16):
      if (_s, _prec) == (512, F16X3):
        continue      # above, with its device step-size twin
      _fc('fused-s%d-%s-b%d' % (_s, PREC_NAME[_prec], _b),
          'run_fused ' + FUSED_OPTIONS[_s][0], 256, _s, _b, _prec,
          route='fused', **FUSED_OPTIONS[_s][1])
  _fc('stream-s2048-bf16x3-warm-b%d' % _b, 'run_stream, warm', 256, 2048, _b,
      BF16X3, warm=True, route='stream')
  _fc('tiled-f32-15x18-b%d' % _b, 'run_generic f32, odd n and s (EpiProx)',
      15, 18, _b, F32, variant=ISTA, warm=True, route='tiled')
  _fc('tiled-f16x3-100x200-b%d' % _b, 'run_generic f16x3, one K slice', 100,
      200, _b, F16X3, route='tiled')
  assert _x3_want_slices(_b, 100, 200) == 1
  _fc('tiled-f16x3-splitK-100x2400-b%d' % _b, 'run_generic split-K slabs',
      100, 2400, _b, F16X3, warm=True, route='tiled')
  _fc('tiled-bf16x3-splitK-100x2400-b%d' % _b,
      'run_generic bf16x3 split-K, state not cleared', 100, 2400, _b, BF16X3,
      route='tiled')
  assert _x3_want_slices(_b, 100, 2400) > 1
  # early stopping (eps = 0 never fires) bypasses every on-chip kernel
  _fc('eps0-f32-256x512-b%d' % _b,
      'early stopping: run_generic, stop accumulator', 256, 512, _b, F32,
      eps=0.0, route='tiled')
  _fc('eps0-f16x3-256x512-b%d' % _b,
      'early stopping on a fused shape: tiled f16x3', 256, 512, _b, F16X3,
      eps=0.0, route='tiled')
  _fc('eps0-f32-64x64-ista-b%d' % _b, 'early stopping bypasses run_small',
      64, 64, _b, F32, variant=ISTA, eps=0.0, route='tiled')
_fc('hard-nonneg-tiled-f32-b33', 'threshold modes in the epilogue', 100, 200,
    33, F32, thr=HARD_NONNEG, route='tiled')


# --------------------------------------------------------- subspace inference
def _tables(groups, s):
  from vtc_hip import groups as vg
  t = vg.GroupTables(groups, s, 'cpu')
  return t, {'index': t.index.numpy(), 'valid': t.valid.numpy(),
             'atom_ptr': t.atom_ptr.numpy(),
             'atom_slots': t.atom_slots.numpy()}


def _regular_groups(count, m):
  return [list(range(m * g, m * g + m)) for g in range(count)]


def _ragged_groups(count, m, s):
  """Groups of 1..m atoms; every third one shares an atom with the previous
  group (overlap), the last atoms of the dictionary are in no group."""
  out, a = [], 0
  for g in range(count):
    size = 1 + (g * 5 + 2) % m if g else m
    members = list(range(a, a + size))
    a += size
    if g % 3 == 2:
      members[0] = out[-1][0]
    out.append(members)
  assert a <= s - 2
  return out


def _subspace(name, branch, n, groups_fn, s, b, prec, variant=FISTA,
              warm=False, eps=-1.0, iters=10, route=None):
  @case('vtc_subspace_ista_fista', name, branch)
  def make(lib):
    groups = groups_fn()
    t, tab = _tables(groups, s)
    G, m, slots = t.num_groups, t.m, t.slots
    rs = np.random.RandomState(slots + b)
    X = helpers.gaussian_patches(slots + b, b, n)
    D = helpers.unit_rows(slots + 3, s, n)
    Dg = (D[tab['index']] * tab['valid'][:, None]).astype(np.float32)
    D64 = torch.from_numpy(D).double()
    dg64 = torch.from_numpy(Dg).double()
    eta = float(np.float32(1.0 / float(sc_oracle.largest_eigenvalue(
        dg64.t() @ dg64))))
    lam = 0.02
    init_atoms = _sparse_codes(rs, (b, s), 0.2) if warm else None
    init = None
    if warm:
      init = (init_atoms[:, tab['index']] * tab['valid'][None, :]).astype(
          np.float32)
    need = lib.vtc_subspace_ista_fista_workspace_bytes(b, n, G, m)

    def call(lib, p, ws, wsb, st):
      done = ctypes.c_int(-1)
      rc = lib.vtc_subspace_ista_fista(
          p['images'], p['grouped_dictionary'], p['initial'], p['codes'], b,
          n, G, m, eta, lam, iters, variant, eps, prec, ws, wsb,
          ctypes.byref(done), st)
      spec.host['iters'] = done.value
      return rc

    def truth(want, inp):
      r = min(b, 64)
      assert spec.host['iters'] == iters
      grouped = want['codes'][:r].astype(np.float64)
      # padding slots hold exact zeros
      assert (want['codes'][:, tab['valid'] == 0] == 0).all()
      summed = np.zeros((r, s))
      for slot in np.nonzero(tab['valid'])[0]:
        summed[:, tab['index'][slot]] += grouped[:, slot]
      ref = sc_oracle.subspace_ista_fista(
          torch.from_numpy(X[:r]).double(), D64, groups, lam, iters,
          variant='fista' if variant == FISTA else 'ista',
          initial_codes=(torch.from_numpy(init_atoms[:r]).double()
                         if warm else None),
          early_stopping_epsilon=None if eps < 0 else float(eps),
          stepsize=eta)
      return _codes_truth(summed, ref.numpy(), prec, 'summed codes')

    # vtc_subspace_ista_fista_workspace_bytes: the larger of the tiled and
    # the streamed need; the runner shows which size check answers
    tiled = _tiled_need(b, n, slots)
    stream_shape = n == 256 and slots % 256 == 0 and m in (1, 2, 4, 8)
    stream = _stream_need(b, slots) if stream_shape else 0
    assert need == max(tiled, stream)
    if route == 'stream':
      assert stream_shape and prec != F32 and eps < 0
      route_need, gate = stream, 'streamed fused FISTA: workspace too small'
    else:
      assert not stream_shape or prec == F32 or eps >= 0
      route_need, gate = tiled, 'vtc_subspace_ista_fista: workspace too small'
    spec = Spec({'images': X, 'grouped_dictionary': Dg, 'initial': init},
                {'codes': ((b, slots), np.float32)}, call, truth,
                ws_bytes=need, need=route_need, gate=gate)
    return spec
  return make


for _b in (1, 33, 130):
  _subspace('tiled-f32-ragged-b%d' % _b,
            'tiled f32, ragged overlapping groups, padding slots', 100,
            lambda: _ragged_groups(30, 4, 120), 120, _b, F32, route='tiled')
  _subspace('tiled-bf16x3-m4-b%d' % _b, 'tiled bf16x3', 100,
            lambda: _regular_groups(50, 4), 200, _b, BF16X3, route='tiled')
  _subspace('tiled-f16x3-m4-b%d' % _b, 'tiled f16x3, prox in the epilogue',
            100, lambda: _regular_groups(50, 4), 200, _b, F16X3, warm=True,
            route='tiled')
  _subspace('tiled-f16x3-m3-b%d' % _b,
            'm = 3: f16x3 falls back to the bf16 split (ADVICE.md)', 256,
            lambda: _regular_groups(128, 3), 384, _b, F16X3, route='tiled')
  for _m in (2, 4, 8):
    _subspace('stream-m%d-b%d' % (_m, _b), 'run_stream group prox m=%d' % _m,
              256, (lambda m=_m: _regular_groups(512 // m, m)), 512, _b,
              F16X3 if _m != 4 else BF16X3, warm=(_m == 8), route='stream')
  _subspace('tiled-f32-eps0-b%d' % _b,
            'early stopping, f32 on a streamed shape', 256,
            lambda: _regular_groups(128, 4), 512, _b, F32, eps=0.0,
            route='tiled')
  _subspace('tiled-f16x3-eps0-ragged-b%d' % _b,
            'early stopping bypasses run_stream; ragged groups', 256,
            lambda: _ragged_groups(128, 4, 512), 512, _b, F16X3, eps=0.0,
            variant=ISTA, route='tiled')


# ------------------------------------------------- group gather / scatter
GROUP_TABLES = {
    'ragged': lambda: (_ragged_groups(30, 4, 120), 120),
    'overlap-wide': lambda: ([[0, 1, 2, 3, 4, 5, 6], [3], [6, 7, 3],
                              [9, 10], [10, 0]], 14),
    'single': lambda: ([[2]], 5),
}


def _group_cases(tag, groups_fn):
  @case('vtc_group_gather_rows', tag, 'one block per slot, padding rows zeroed')
  def rows(lib):
    groups, s = groups_fn()
    t, tab = _tables(groups, s)
    n = 37
    D = np.random.RandomState(s).randn(s, n).astype(np.float32)

    def call(lib, p, ws, wsb, st):
      return lib.vtc_group_gather_rows(p['d'], p['index'], p['valid'],
                                       p['out'], t.slots, n, st)

    def truth(want, inp):
      return [_exact('rows', want['out'],
                     D[tab['index']] * tab['valid'][:, None])]
    return Spec({'d': D, 'index': tab['index'], 'valid': tab['valid']},
                {'out': ((t.slots, n), np.float32)}, call, truth)

  for b in (1, 33):
    @case('vtc_group_gather_cols', '%s-b%d' % (tag, b), 'flat grid over b*slots')
    def cols(lib, b=b):
      groups, s = groups_fn()
      t, tab = _tables(groups, s)
      C = np.random.RandomState(s + b).randn(b, s).astype(np.float32)

      def call(lib, p, ws, wsb, st):
        return lib.vtc_group_gather_cols(p['c'], p['index'], p['valid'],
                                         p['out'], b, s, t.slots, st)

      def truth(want, inp):
        return [_exact('cols', want['out'],
                       C[:, tab['index']] * tab['valid'][None, :])]
      return Spec({'c': C, 'index': tab['index'], 'valid': tab['valid']},
                  {'out': ((b, t.slots), np.float32)}, call, truth)

    @case('vtc_group_scatter_add', '%s-b%d' % (tag, b),
          'CSR walk per (row, atom); atoms in no group get 0')
    def scatter(lib, b=b):
      groups, s = groups_fn()
      t, tab = _tables(groups, s)
      Gc = np.random.RandomState(s + b + 1).randn(b, t.slots).astype(
          np.float32)

      def call(lib, p, ws, wsb, st):
        return lib.vtc_group_scatter_add(p['g'], p['atom_ptr'],
                                         p['atom_slots'], p['out'], b, s,
                                         t.slots, st)

      def truth(want, inp):
        ref = np.zeros((b, s), np.float32)     # float32 adds in slot order
        for a in range(s):
          for k in range(tab['atom_ptr'][a], tab['atom_ptr'][a + 1]):
            ref[:, a] = ref[:, a] + Gc[:, tab['atom_slots'][k]]
        return [_exact('scatter', want['out'], ref)]
      return Spec({'g': Gc, 'atom_ptr': tab['atom_ptr'],
                   'atom_slots': tab['atom_slots']},
                  {'out': ((b, s), np.float32)}, call, truth)

    @case('vtc_group_norm_sum', '%s-b%d' % (tag, b),
          'groups strided over 256 threads')
    def norm_sum(lib, b=b):
      groups, s = groups_fn()
      t, tab = _tables(groups, s)
      C = np.random.RandomState(s + b + 2).randn(b, s).astype(np.float32)

      def call(lib, p, ws, wsb, st):
        return lib.vtc_group_norm_sum(p['c'], p['index'], p['valid'],
                                      p['out'], b, s, t.num_groups, t.m, st)

      def truth(want, inp):
        sq = (C.astype(np.float64)[:, tab['index']] ** 2 *
              tab['valid'][None, :]).reshape(b, t.num_groups, t.m)
        norms = np.sqrt(sq.sum(axis=2))
        # each norm: m fused squares, one sqrt; then a G-term sum
        bound = (t.num_groups + t.m + 1) * U24 * norms.sum(axis=1)
        return [_elementwise('norm sum', want['out'], norms.sum(axis=1),
                             bound)]
      return Spec({'c': C, 'index': tab['index'], 'valid': tab['valid']},
                  {'out': ((b,), np.float32)}, call, truth)


for _tag, _fn in sorted(GROUP_TABLES.items()):
  _group_cases(_tag, _fn)


@case('vtc_group_norm_sum', 'many-groups-b3', '700 groups: > 256 per block')
def _norm_sum_many(lib):
  groups, s, b = _regular_groups(700, 2), 1400, 3
  t, tab = _tables(groups, s)
  C = np.random.RandomState(9).randn(b, s).astype(np.float32)

  def call(lib, p, ws, wsb, st):
    return lib.vtc_group_norm_sum(p['c'], p['index'], p['valid'], p['out'],
                                  b, s, 700, 2, st)

  def truth(want, inp):
    norms = np.sqrt((C.astype(np.float64) ** 2).reshape(b, 700, 2).sum(2))
    return [_elementwise('norm sum', want['out'], norms.sum(1),
                         (700 + 3) * U24 * norms.sum(1))]
  return Spec({'c': C, 'index': tab['index'], 'valid': tab['valid']},
              {'out': ((b,), np.float32)}, call, truth)


# ------------------------------------------------------------- convolutional
def _conv_route(g):
  """tests/test_large_batch_gpu.py::_conv_route on a dict geometry."""
  ch = (g['h'] - g['kh']) // g['stride_v'] + 1
  cw = (g['w'] - g['kw']) // g['stride_h'] + 1
  cover = _ceil(g['kh'], g['stride_v']) * _ceil(g['kw'], g['stride_h'])
  if ((g['stride_v'] > 1 or g['stride_h'] > 1) and cover <= 16 and
      g['c'] * g['kh'] * g['kw'] <= 8192 and g['b'] <= 65535 and
      g['b'] * ch * cw < (1 << 31)):
    return 'patch'
  unit = (g['stride_v'] == 1 and g['stride_h'] == 1 and g['kh'] == g['kw']
          and g['kh'] in (5, 8, 11, 16))
  wy, wx = 32 + g['kh'] - 1, (64 + g['kw'] - 1 + 3) // 4 * 4
  fits = (g['c'] * wy * wx + g['s'] * g['c'] * g['kh'] *
          ((g['kw'] + 3) // 4 * 4)) * 4 <= 140 * 1024
  return 'unit' if unit and fits else 'direct'


def _conv_setup(b, c, size_h, size_w, s, k, stride, has_padding, seed):
  """Geometry, padded images (zero frame), unit-norm kernels, padding dims."""
  rs = np.random.RandomState(seed)
  if has_padding:
    lv, tv = sc_oracle.conv_padding_amount(size_h, k, stride)
    lh, th = sc_oracle.conv_padding_amount(size_w, k, stride)
  else:
    # no padding: trim the image so that (code - 1) * stride + k covers it
    size_h -= (size_h - k) % stride
    size_w -= (size_w - k) % stride
    lv = tv = lh = th = 0
  H, W = size_h + lv + tv, size_w + lh + th
  imgs = np.zeros((b, c, H, W), np.float32)
  imgs[:, :, lv:lv + size_h, lh:lh + size_w] = (
      0.5 * rs.randn(b, c, size_h, size_w)).astype(np.float32)
  D = rs.randn(s, c, k, k).astype(np.float32)
  D /= np.sqrt((D.astype(np.float64) ** 2).sum(axis=(1, 2, 3)))[
      :, None, None, None].astype(np.float32)
  g = dict(b=b, c=c, h=H, w=W, s=s, kh=k, kw=k, stride_v=stride,
           stride_h=stride, has_padding=1 if has_padding else 0,
           pad_lead_v=lv, pad_trail_v=tv, pad_lead_h=lh, pad_trail_h=th)
  pad = ((lv, tv), (lh, th)) if has_padding else None
  ch = (H - k) // stride + 1
  cw = (W - k) // stride + 1
  return g, imgs, D, pad, ch, cw


def _conv(name, branch, c, size, s, k, stride, prec, route, fused=None, b=2,
          has_padding=True, warm=False, variant=FISTA, iters=8, eps=-1.0):
  @case('vtc_conv_ista_fista', name, branch)
  def make(lib):
    g, imgs, D, pad, ch, cw = _conv_setup(b, c, size[0], size[1], s, k,
                                          stride, has_padding, 50 + k + s)
    geom = _geom(g)
    cover = _ceil(k, stride) ** 2
    eta = float(np.float32(float(sc_oracle.conv_stepsize(
        torch.from_numpy(D).double())) / cover))
    lam = 0.05
    rs = np.random.RandomState(k + s)
    init = _sparse_codes(rs, (b, s, ch, cw), 0.05, 0.1) if warm else None
    need = lib.vtc_conv_ista_fista_workspace_bytes(ctypes.byref(geom))

    def call(lib, p, ws, wsb, st):
      done = ctypes.c_int(-1)
      rc = lib.vtc_conv_ista_fista(
          p['images'], p['dictionary'], p['initial'], p['codes'],
          ctypes.byref(geom), eta, lam, iters, variant, SOFT, eps, prec, ws,
          wsb, ctypes.byref(done), st)
      spec.host['iters'] = done.value
      return rc

    def truth(want, inp):
      assert spec.host['iters'] == iters
      ref = sc_oracle.conv_ista_fista(
          torch.from_numpy(imgs).double(), torch.from_numpy(D).double(),
          (stride, stride), pad, lam, iters,
          variant='fista' if variant == FISTA else 'ista',
          initial_codes=(torch.from_numpy(init).double() if warm else None),
          early_stopping_epsilon=None if eps < 0 else float(eps),
          stepsize=eta)
      return _codes_truth(want['codes'], ref.numpy(), prec, 'codes')

    def check_route(lib):
      x3 = bool(lib.vtc_conv_x3_supported(ctypes.byref(geom)))
      # conv_inference_ws term by term; what is left over is the split-mode
      # operand images and, only where the fused iteration kernel runs, its
      # two code maps in fragment order (cx_fused_bytes): the query itself
      # tells the fused from the two-kernel plan
      code_bytes = 4 * b * s * ch * cw
      ctaps = c * k * k
      base = (3 * _au(code_bytes) + _au(8 * 4 * b * c * g['h'] * g['w']) +
              _au(4 * s * ctaps) + _au(4 * (64 + 4 * b)) + 256)
      patch = 2 * _au(4 * b * ch * cw * ctaps)
      is_patch = _conv_route(g) == 'patch'
      split_bytes = need - base - (patch if is_patch else 0)
      assert split_bytes >= 0
      assert (split_bytes > 0) == x3
      if prec == F32:
        assert _conv_route(g) == route, _conv_route(g)
        assert (route == 'patch') == (need - base >= patch)
      else:
        assert x3 and fused == (split_bytes >= 2 * code_bytes), split_bytes
      assert (g['h'] % 32, g['w'] % 64) != (0, 0)

    spec = Spec({'images': imgs, 'dictionary': D, 'initial': init},
                {'codes': ((b, s, ch, cw), np.float32)}, call, truth,
                ws_bytes=need, tight=True, route=check_route)
    return spec
  return make


_conv('patch-k8-s4', 'patch route: im2col + contributions', 1, (70, 93), 16,
      8, 4, F32, 'patch')
_conv('patch-k8-s4-c3-nopad-warm', 'patch route, c = 3, mask of ones', 3,
      (70, 93), 16, 8, 4, F32, 'patch', has_padding=False, warm=True)
_conv('unit-k11-f32', 'unit route: stride-1 direct kernels, partials', 1,
      (70, 93), 16, 11, 1, F32, 'unit')
_conv('unit-k11-f32-nopad-ista', 'unit route without padding, ISTA warm', 1,
      (70, 93), 16, 11, 1, F32, 'unit', has_padding=False, warm=True,
      variant=ISTA)
_conv('direct-k16-s2', 'general direct kernels', 1, (70, 93), 16, 16, 2, F32,
      'direct')
_conv('direct-k16-s2-eps0', 'direct kernels with the stop accumulator', 1,
      (40, 51), 8, 16, 2, F32, 'direct', eps=0.0)
_conv('fused-x3-k11-f16x3', 'fused x3 kernel: synp image, Cfrag maps', 1,
      (70, 93), 48, 11, 1, F16X3, None, fused=True)
_conv('fused-x3-k11-bf16x3-warm', 'fused x3 kernel, bf16 split, warm', 1,
      (70, 93), 48, 11, 1, BF16X3, None, fused=True, warm=True)
_conv('fused-x3-k11-f16x3-nopad', 'fused x3 kernel, mask of ones', 1,
      (70, 93), 48, 11, 1, F16X3, None, fused=True, has_padding=False)
_conv('two-kernel-x3-k16-f16x3', 'two-kernel x3: k = 16', 1, (70, 93), 16, 16,
      1, F16X3, None, fused=False)
_conv('two-kernel-x3-k11-c3-bf16x3', 'two-kernel x3: c = 3', 3, (70, 93), 48,
      11, 1, BF16X3, None, fused=False)
_conv('two-kernel-x3-k11-s16-f16x3-warm', 'two-kernel x3: s <= 32', 1,
      (70, 93), 16, 11, 1, F16X3, None, fused=False, warm=True)

CONV_UPDATE_GEOMS = {
    'patch': (1, (38, 45), 8, 8, 4),
    'unit': (1, (38, 45), 8, 11, 1),
    'direct': (1, (38, 45), 8, 16, 2),
}


def _conv_codes(rs, b, s, ch, cw):
  return _sparse_codes(rs, (b, s, ch, cw), 0.1, 0.3)


def _conv_update(tag, c, size, s, k, stride, prec, b=3):
  def residual(lib):
    g, imgs, D, pad, ch, cw = _conv_setup(b, c, size[0], size[1], s, k,
                                          stride, True, 70 + k)
    geom = _geom(g)
    C = _conv_codes(np.random.RandomState(k), b, s, ch, cw)

    def call(lib, p, ws, wsb, st):
      return lib.vtc_conv_residual(p['images'], p['dictionary'], p['codes'],
                                   p['residual'], ctypes.byref(geom), st)

    def truth(want, inp):
      x = torch.from_numpy(imgs).double()
      cc, dd = torch.from_numpy(C).double(), torch.from_numpy(D).double()
      ref = sc_oracle.conv_mask(x, pad) * (
          sc_oracle.conv_synthesis(cc, dd, (stride, stride)) - x)
      mag = sc_oracle.conv_synthesis(cc.abs(), dd.abs(),
                                     (stride, stride)) + x.abs()
      terms = s * _ceil(k, stride) ** 2 + 1
      return [_elementwise('residual', want['residual'], ref.numpy(),
                           terms * U24 * mag.numpy())]
    return Spec({'images': imgs, 'dictionary': D, 'codes': C},
                {'residual': (imgs.shape, np.float32)}, call, truth)
  if prec == F32:
    case('vtc_conv_residual', tag, 'residual, %s geometry' % tag)(residual)

  @case('vtc_conv_dict_gradient', '%s-%s' % (tag, PREC_NAME[prec]),
        'gradient, %s geometry' % tag)
  def gradient(lib):
    g, imgs, D, pad, ch, cw = _conv_setup(b, c, size[0], size[1], s, k,
                                          stride, True, 70 + k)
    geom = _geom(g)
    C = _conv_codes(np.random.RandomState(k), b, s, ch, cw)
    need = lib.vtc_conv_dict_gradient_workspace_bytes(ctypes.byref(geom))

    def call(lib, p, ws, wsb, st):
      return lib.vtc_conv_dict_gradient(
          p['images'], p['dictionary'], p['codes'], p['grad'],
          ctypes.byref(geom), prec, ws, wsb, st)

    def truth(want, inp):
      ref = update_oracle.conv_gradient_sum(
          torch.from_numpy(imgs), torch.from_numpy(D), torch.from_numpy(C),
          (stride, stride), pad)
      # REL_TOL_DICT cannot be met by a bf16 split (2^-17 per product): the
      # split route keeps the gate the suite already holds it to
      tol = (helpers.REL_TOL_DICT if prec == F32
             else update_oracle.GRAD_GATES['conv-bf16x3'])
      return [('grad_sum', update_oracle.rel(torch.from_numpy(want['grad']),
                                             ref), tol)]

    def route(lib):
      if prec != F32:
        assert lib.vtc_conv_x3_supported(ctypes.byref(geom))
      else:
        assert _conv_route(g) == tag.split('-')[0]
    return Spec({'images': imgs, 'dictionary': D, 'codes': C},
                {'grad': (D.shape, np.float32)}, call, truth, ws_bytes=need,
                tight=True, route=route)


for _tag, (_c, _size, _s, _k, _stride) in sorted(CONV_UPDATE_GEOMS.items()):
  _conv_update(_tag, _c, _size, _s, _k, _stride, F32)
_conv_update('unit', 1, (38, 45), 8, 11, 1, BF16X3)


def _conv_apply(name, s, c, k, hessian, normalize):
  @case('vtc_conv_dict_apply', name, 'scratch of exactly s * kernel_elems '
        'floats')
  def make(lib):
    rs = np.random.RandomState(s + k)
    ke = c * k * k
    D = rs.randn(s, c, k, k).astype(np.float32)
    D /= np.sqrt((D.astype(np.float64) ** 2).sum(axis=(1, 2, 3)))[
        :, None, None, None].astype(np.float32)
    grad = rs.randn(s, c, k, k).astype(np.float32)
    hess = (0.5 + rs.rand(s)).astype(np.float32) if hessian else None
    batch, step = 7, 0.03

    def call(lib, p, ws, wsb, st):
      # the scratch is this entry point's workspace: fenced at exactly
      # s * kernel_elems floats
      return lib.vtc_conv_dict_apply(
          p['dictionary'], p['grad'], p['hessian'], batch, step,
          update_oracle.LOWEST_CODE_VAL, 1 if normalize else 0, s, ke, ws, st)

    def truth(want, inp):
      ref = update_oracle.conv_apply(
          torch.from_numpy(D), torch.from_numpy(grad), batch, step,
          torch.from_numpy(hess) if hessian else None, normalize)
      return [('dictionary', update_oracle.rel(
          torch.from_numpy(want['dictionary']), ref), helpers.REL_TOL_DICT)]
    return Spec({'dictionary': D, 'grad': grad, 'hessian': hess}, {}, call,
                truth, ws_bytes=4 * s * ke, inout=('dictionary',))
  return make


_conv_apply('k8-hessian', 8, 1, 8, True, True)
_conv_apply('k11-c3-plain', 5, 3, 11, False, True)
_conv_apply('k16-s33-unnormalised', 33, 1, 16, True, False)


# -------------------------------------------------- fully-connected updates
UPDATE_SHAPES = ((1, 16, 6), (257, 100, 200), (8192, 256, 1024))


def _fc_update(b, n, s):
  tag = 'b%d-n%d-s%d' % (b, n, s)

  def data():
    rs = np.random.RandomState(b + n + s)
    X = helpers.gaussian_patches(b + n, b, n)
    D = helpers.unit_rows(s + n, s, n)
    C = _sparse_codes(rs, (b, s), 0.2, 0.2)
    return X, D, C

  @case('vtc_fc_dict_gradient', tag, 'residual in the workspace, C^T R')
  def gradient(lib):
    X, D, C = data()
    need = lib.vtc_fc_dict_gradient_workspace_bytes(b, n, s)

    def call(lib, p, ws, wsb, st):
      return lib.vtc_fc_dict_gradient(p['x'], p['d'], p['c'], p['grad'], b, n,
                                      s, ws, wsb, st)

    def truth(want, inp):
      ref = update_oracle.fc_gradient_sum(
          torch.from_numpy(X), torch.from_numpy(D), torch.from_numpy(C))
      return [('grad_sum', update_oracle.rel(torch.from_numpy(want['grad']),
                                             ref), helpers.REL_TOL_DICT)]
    return Spec({'x': X, 'd': D, 'c': C}, {'grad': ((s, n), np.float32)},
                call, truth, ws_bytes=need, tight=True)

  @case('vtc_fc_residual', tag, 'ragged 128 x 128 / 32 x 32 tiles')
  def residual(lib):
    X, D, C = data()

    def call(lib, p, ws, wsb, st):
      return lib.vtc_fc_residual(p['x'], p['d'], p['c'], p['r'], b, n, s, st)

    def truth(want, inp):
      c64, d64 = C.astype(np.float64), D.astype(np.float64)
      ref = c64 @ d64 - X
      mag = np.abs(c64) @ np.abs(d64) + np.abs(X)
      return [_elementwise('residual', want['r'], ref, (s + 1) * U24 * mag)]
    return Spec({'x': X, 'd': D, 'c': C}, {'r': ((b, n), np.float32)}, call,
                truth)

  for hessian, penalty, normalize in ((True, True, True),
                                      (False, False, False)):
    name = '%s-%s' % (tag, 'full' if hessian else 'plain')

    @case('vtc_fc_dict_apply', name, 'in place, row normalisation')
    def apply_(lib, hessian=hessian, penalty=penalty, normalize=normalize):
      rs = np.random.RandomState(s + n + 1)
      D = helpers.unit_rows(s + n, s, n)
      grad = rs.randn(s, n).astype(np.float32)
      hess = (0.5 + rs.rand(s)).astype(np.float32) if hessian else None
      pen = rs.randn(s, n).astype(np.float32) if penalty else None
      batch, step, ap = max(b, 1), 0.05, 0.3

      def call(lib, p, ws, wsb, st):
        return lib.vtc_fc_dict_apply(
            p['dictionary'], p['grad'], p['hessian'], p['penalty'], ap, batch,
            step, update_oracle.LOWEST_CODE_VAL, 1 if normalize else 0, s, n,
            st)

      def truth(want, inp):
        ref = update_oracle.fc_apply(
            torch.from_numpy(D), torch.from_numpy(grad), batch, step,
            torch.from_numpy(hess) if hessian else None,
            torch.from_numpy(pen) if penalty else None, ap, normalize)
        return [('dictionary', update_oracle.rel(
            torch.from_numpy(want['dictionary']), ref),
                 helpers.REL_TOL_DICT)]
      return Spec({'dictionary': D, 'grad': grad, 'hessian': hess,
                   'penalty': pen}, {}, call, truth, inout=('dictionary',))

  for positions in (1, 17 * 23):
    if positions > 1 and b > 257:
      continue        # 8192 x 1024 x 391 floats: not a shape of this engine
    bb = b if positions == 1 else min(b, 5)
    name = '%s-p%d' % (tag, positions)

    @case('vtc_code_energy', name, 'partial sums in the workspace')
    def energy(lib, positions=positions, bb=bb):
      rs = np.random.RandomState(bb + s + positions)
      C = _sparse_codes(rs, (bb, s, positions), 0.3, 0.5)
      need = lib.vtc_code_energy_workspace_bytes(bb, s, positions)

      def call(lib, p, ws, wsb, st):
        return lib.vtc_code_energy(p['c'], bb, s, positions, p['e'], ws, wsb,
                                   st)

      def truth(want, inp):
        sq = (C.astype(np.float64) ** 2).transpose(1, 0, 2).reshape(s, -1)
        return [_elementwise('energy', want['e'], sq.sum(1), _sum_bound(sq))]
      return Spec({'c': C}, {'e': ((s,), np.float32)}, call, truth,
                  ws_bytes=need, tight=True)

  @case('vtc_hessian_ema', tag, 'in place, s elements')
  def ema(lib):
    rs = np.random.RandomState(s)
    h = (0.1 + rs.rand(s)).astype(np.float32)
    e = (rs.rand(s) * b).astype(np.float32)

    def call(lib, p, ws, wsb, st):
      return lib.vtc_hessian_ema(p['h'], p['e'], b, s, st)

    def truth(want, inp):
      a, c = 0.99 * h.astype(np.float64), e.astype(np.float64) / b / 100
      # three float32 roundings of the terms and one of the sum
      return [_elementwise('hessian', want['h'], a + c, 4 * U24 * (a + c))]
    return Spec({'h': h, 'e': e}, {}, call, truth, inout=('h',))

  for sq in (min(n, s),):     # ICA dictionaries are square

    @case('vtc_ica_moment', 'b%d-s%d' % (b, sq), 'codes^T sign(codes)')
    def moment(lib, sq=sq):
      C = np.random.RandomState(b + sq).laplace(size=(b, sq)).astype(
          np.float32)
      need = lib.vtc_ica_moment_workspace_bytes(b, sq)

      def call(lib, p, ws, wsb, st):
        return lib.vtc_ica_moment(p['c'], p['m'], b, sq, ws, wsb, st)

      def truth(want, inp):
        c64 = C.astype(np.float64)
        ref = c64.T @ np.sign(c64)
        bound = b * U24 * (np.abs(c64).T @ np.abs(np.sign(c64)))
        return [_elementwise('moment', want['m'], ref, bound)]
      return Spec({'c': C}, {'m': ((sq, sq), np.float32)}, call, truth,
                  ws_bytes=need, tight=True)

    @case('vtc_ica_apply', 'b%d-s%d' % (b, sq), 'D += step (M / b - I) D')
    def ica_apply(lib, sq=sq):
      rs = np.random.RandomState(sq + 5)
      D = helpers.unit_rows(sq + 2, sq, sq)
      M = (b * (np.eye(sq) + 0.1 * rs.randn(sq, sq))).astype(np.float32)
      step = 0.1
      need = lib.vtc_ica_apply_workspace_bytes(sq, sq)

      def call(lib, p, ws, wsb, st):
        return lib.vtc_ica_apply(p['d'], p['m'], b, sq, sq, step, ws, wsb, st)

      def truth(want, inp):
        d64 = D.astype(np.float64)
        ref = d64 + step * ((M.astype(np.float64) / b - np.eye(sq)) @ d64)
        return [('dictionary', helpers.rel_err(want['d'], ref),
                 helpers.REL_TOL_DICT)]
      return Spec({'d': D, 'm': M}, {}, call, truth, ws_bytes=need,
                  tight=True, inout=('d',))


for _shape in UPDATE_SHAPES:
  _fc_update(*_shape)


def _alignment(name, groups_fn, s, n, normalized):
  @case('vtc_subspace_alignment_gradient', name, 'one LDS tile per group')
  def make(lib):
    groups = groups_fn()
    t, tab = _tables(groups, s)
    D = helpers.unit_rows(s + n, s, n)
    if not normalized:
      D = (D * (0.5 + np.random.RandomState(1).rand(s, 1))).astype(np.float32)
    need = lib.vtc_subspace_alignment_gradient_workspace_bytes(t.slots, n)

    def call(lib, p, ws, wsb, st):
      return lib.vtc_subspace_alignment_gradient(
          p['d'], p['index'], p['valid'], p['atom_ptr'], p['atom_slots'],
          p['out'], s, n, t.num_groups, t.m, 1 if normalized else 0, ws, wsb,
          st)

    def truth(want, inp):
      ref = update_oracle.alignment_gradient_sum(torch.from_numpy(D), groups,
                                                 normalized)
      # relative to the gradient; where the reference is zero by construction
      # (a group of one atom has no pair) relative to the dictionary it is
      # subtracted from
      d_norm = float(np.linalg.norm(D.astype(np.float64)))
      scale = float(ref.norm())
      if scale <= 1e-6 * d_norm:
        scale = d_norm
      err = float((torch.from_numpy(want['out']).double() - ref).norm())
      return [('penalty_grad', err / scale, helpers.REL_TOL_DICT)]
    return Spec({'d': D, 'index': tab['index'], 'valid': tab['valid'],
                 'atom_ptr': tab['atom_ptr'],
                 'atom_slots': tab['atom_slots']},
                {'out': ((s, n), np.float32)}, call, truth, ws_bytes=need,
                tight=True)
  return make


_alignment('groups-of-1', lambda: _regular_groups(16, 1), 16, 6, True)
_alignment('groups-of-8', lambda: _regular_groups(25, 8), 200, 100, True)
_alignment('ragged-unnormalised', lambda: _ragged_groups(30, 4, 120), 120,
           100, False)
_alignment('groups-of-8-n256', lambda: _regular_groups(128, 8), 1024, 256,
           True)


# ------------------------------------------------------------ Lipschitz step
def _gram(rows, cols, transpose_a):
  @case('vtc_gram', '%dx%d-t%d' % (rows, cols, transpose_a),
        'A^T A' if transpose_a else 'A A^T')
  def make(lib):
    A = np.random.RandomState(rows + cols).randn(rows, cols).astype(
        np.float32)
    side = cols if transpose_a else rows

    def call(lib, p, ws, wsb, st):
      return lib.vtc_gram(p['a'], rows, cols, transpose_a, p['g'], st)

    def truth(want, inp):
      a = A.astype(np.float64)
      ref = a.T @ a if transpose_a else a @ a.T
      mag = np.abs(a).T @ np.abs(a) if transpose_a else np.abs(a) @ np.abs(a).T
      k = rows if transpose_a else cols
      return [_elementwise('gram', want['g'], ref, k * U24 * mag)]
    return Spec({'a': A}, {'g': ((side, side), np.float32)}, call, truth)
  return make


for _shape in ((50, 36), (1024, 256)):
  for _t in (0, 1):
    _gram(_shape[0], _shape[1], _t)


def _lambda_max(n, mirrored):
  entry = 'vtc_lambda_max_mirrored' if mirrored else 'vtc_lambda_max'

  @case(entry, 'n%d' % n, 'no workspace' if n <= 256 else
        'Krylov basis in the workspace')
  def make(lib):
    rs = np.random.RandomState(n)
    A = rs.randn(max(n // 2, 1) + 3, n)
    G = (A.T @ A).astype(np.float32)
    G = ((G + G.T) / 2).astype(np.float32)
    query = lib.vtc_lambda_max_workspace_bytes(n)
    # n <= 256: the query answers with a token 256 bytes, the header says the
    # call needs none -- the fenced call passes (NULL, 0)
    need = query if n > 256 else 0

    def call(lib, p, ws, wsb, st):
      if mirrored:
        pinned = torch.full((3,), float('nan')).pin_memory()
        rc = lib.vtc_lambda_max_mirrored(
            p['g'], n, p['out'], ctypes.c_void_p(pinned.data_ptr()), ws, wsb,
            st)
        torch.cuda.synchronize()
        spec.host['mirror'] = pinned.tolist()
        return rc
      return lib.vtc_lambda_max(p['g'], n, p['out'], ws, wsb, st)

    def truth(want, inp):
      lam, inv, conv = [float(v) for v in want['out']]
      ref = float(np.linalg.eigvalsh(G.astype(np.float64))[-1])
      assert conv == 1.0
      if mirrored:
        assert spec.host['mirror'] == [lam, inv, conv]
      # tests/test_lipschitz_gpu.py gates the solve at 2e-6 relative
      return [('lambda_max', abs(lam - ref) / ref, 2e-6),
              ('1 / lambda_max', abs(inv - 1 / ref) * ref, 2e-6)]

    def route(lib):
      assert (query <= 256) == (n <= 256)   # the Krylov basis: 4 n floats up
    spec = Spec({'g': G}, {'out': ((3,), np.float32)}, call, truth,
                ws_bytes=need, tight=n > 256, need=None if n > 256 else 0,
                route=route)
    return spec
  return make


for _n in (1, 64, 256, 257, 1024):
  _lambda_max(_n, False)
for _n in (64, 1024):
  _lambda_max(_n, True)


# ------------------------------------------------------------------- metrics
STAT_COLS = (1, 63, 64, 65, 255, 256, 257, 100003)


def _stat_rows(cols, rows=3):
  rs = np.random.RandomState(cols)
  x = rs.randn(rows, cols).astype(np.float32)
  x[rs.rand(rows, cols) < 0.3] = 0.0
  flat = x.reshape(-1)
  flat[::7] = -0.0                       # not counted by l0
  flat[3::11] = np.float32(1e-40)        # denormal: counted, squares to 0
  flat[5::13] = np.float32(-3e-42)
  return x


def _row_stats(cols, null):
  @case('vtc_row_stats', 'cols%d-null-%s' % (cols, null or 'none'),
        'block of 256 strided over the row')
  def make(lib):
    x = _stat_rows(cols)
    rows = x.shape[0]
    outs = {k: (None if k == null else ((rows,), np.float32))
            for k in ('sumsq', 'l1', 'l0')}

    def call(lib, p, ws, wsb, st):
      return lib.vtc_row_stats(p['x'], rows, cols, p['sumsq'], p['l1'],
                               p['l0'], st)

    def truth(want, inp):
      x64 = x.astype(np.float64)
      out = []
      if null != 'sumsq':
        out.append(_elementwise('sumsq', want['sumsq'], (x64 ** 2).sum(1),
                                _sum_bound(x64 ** 2)))
      if null != 'l1':
        out.append(_elementwise('l1', want['l1'], np.abs(x64).sum(1),
                                _sum_bound(x64)))
      if null != 'l0':
        out.append(_exact('l0', want['l0'],
                          (x != 0).sum(1).astype(np.float32)))
      return out
    return Spec({'x': x}, outs, call, truth)
  return make


for _cols in STAT_COLS:
  _row_stats(_cols, None)
for _null in ('sumsq', 'l1', 'l0'):
  _row_stats(65, _null)
  _row_stats(257, _null)


def _mean_abs_diff(cols):
  @case('vtc_rows_mean_abs_diff', 'cols%d' % cols, 'block of 256 per row')
  def make(lib):
    rs = np.random.RandomState(cols + 1)
    a = rs.randn(3, cols).astype(np.float32)
    b = rs.randn(3, cols).astype(np.float32)

    def call(lib, p, ws, wsb, st):
      return lib.vtc_rows_mean_abs_diff(p['a'], p['b'], 3, cols, p['out'], st)

    def truth(want, inp):
      d = np.abs(a.astype(np.float64) - b.astype(np.float64))
      return [_elementwise('mean', want['out'], d.mean(1),
                           _sum_bound(d) / cols)]
    return Spec({'a': a, 'b': b}, {'out': ((3,), np.float32)}, call, truth)
  return make


for _cols in STAT_COLS:
  _mean_abs_diff(_cols)


def _window(name, stack, origin, window, branch):
  @case('vtc_window_minmax', name, branch)
  def make(lib):
    o, h, w = stack
    wo, wr, wc = window
    o0, r0, c0 = origin
    rs = np.random.RandomState(o * h * w)
    x = rs.randn(o, h, w).astype(np.float32)
    # the extremes of the stack sit just outside the window
    if c0 > 0:
      x[o0, r0, c0 - 1] = 100.0
    if c0 + wc < w:
      x[o0, r0, c0 + wc] = -100.0
    if r0 > 0:
      x[o0, r0 - 1, c0] = -200.0
    if r0 + wr < h:
      x[o0, r0 + wr, c0] = 200.0
    offset = (o0 * h + r0) * w + c0
    need = lib.vtc_window_minmax_workspace_bytes()

    def call(lib, p, ws, wsb, st):
      base = ctypes.c_void_p(p['x'].value + 4 * offset)
      return lib.vtc_window_minmax(base, wo, wr, wc, h * w, w, p['out'], ws,
                                   wsb, st)

    def truth(want, inp):
      win = x[o0:o0 + wo, r0:r0 + wr, c0:c0 + wc]
      return [_exact('min max', want['out'],
                     np.array([win.min(), win.max()], np.float32))]
    return Spec({'x': x}, {'out': ((2,), np.float32)}, call, truth,
                ws_bytes=need, tight=True)
  return make


_window('interior-3x40x56', (3, 40, 56), (0, 5, 7), (3, 30, 41),
        'pitches larger than the window')
_window('one-element', (3, 40, 56), (1, 20, 20), (1, 1, 1), 'one block')
_window('large-2x400x500', (2, 400, 500), (0, 1, 1), (2, 390, 490),
        'more than 512 x 256 elements: grid-stride partials')


# ------------------------------------------------------------ patch pipeline
def _whiten(h, w, c, norm_and_threshold, count=2):
  @case('vtc_whiten_center_surround', '%dx%dx%d-nt%d' % (h, w, c,
                                                         norm_and_threshold),
        'float64 FFT planes in the workspace')
  def make(lib):
    rs = np.random.RandomState(h * w + c)
    x = rs.rand(count, h, w, c).astype(np.float32)
    lo, hi = 1e-3, 0.9
    need = lib.vtc_whiten_center_surround_workspace_bytes(count, h, w, c)

    def call(lib, p, ws, wsb, st):
      return lib.vtc_whiten_center_surround(
          p['x'], p['out'], count, h, w, c, lo, hi, norm_and_threshold, ws,
          wsb, st)

    def truth(want, inp):
      # utils/image_processing.py:219-221,255-264,298: the ramp max(|f|, low)
      # times the low-pass exp(-(|f| / (high / 2))^8) on the fft frequency
      # grid, optionally divided by its maximum and floored at 1e-3
      fy = np.fft.fftfreq(h)[:, None]
      fx = np.fft.fftfreq(w)[None, :]
      rho = np.sqrt(fy ** 2 + fx ** 2)
      lo64, hi64 = float(np.float32(lo)), float(np.float32(hi))
      filt = np.maximum(rho, lo64) * np.exp(-(rho / (0.5 * hi64)) ** 8)
      if norm_and_threshold:
        filt = filt / filt.max()
        filt[filt < 1e-3] = 1e-3
      ref = np.real(np.fft.ifft2(np.fft.fft2(
          x.astype(np.float64), axes=(1, 2)) * filt[None, :, :, None],
          axes=(1, 2)))
      # tests/test_patches_gpu.py gates this transform at 1e-6 relative
      return [('whitened', helpers.rel_err(want['out'], ref), 1e-6)]
    return Spec({'x': x}, {'out': ((count, h, w, c), np.float32)}, call,
                truth, ws_bytes=need, tight=True)
  return make


for _hwc in ((48, 64, 1), (37, 53, 3), (5, 7, 2)):
  for _nt in (0, 1):
    _whiten(_hwc[0], _hwc[1], _hwc[2], _nt)


def _standardize(count):
  @case('vtc_standardize_data_range', 'count%d' % count,
        'min / max partials in the workspace')
  def make(lib):
    x = np.random.RandomState(count).randn(count).astype(np.float32)
    need = lib.vtc_window_minmax_workspace_bytes()

    def call(lib, p, ws, wsb, st):
      return lib.vtc_standardize_data_range(p['x'], p['out'], count, p['mm'],
                                            ws, wsb, st)

    def truth(want, inp):
      lo, hi = x.min(), x.max()
      x64 = x.astype(np.float64)
      ref = (x64 - lo) / (float(hi) - float(lo))
      # three float32 roundings: x - min, max - min, the quotient
      return [_exact('min max', want['mm'], np.array([lo, hi], np.float32)),
              _elementwise('standardized', want['out'], ref,
                           3 * U24 * np.abs(ref) + TINY)]
    return Spec({'x': x}, {'out': ((count,), np.float32),
                           'mm': ((2,), np.float32)}, call, truth,
                ws_bytes=need, tight=True)
  return make


for _count in (2, 1000, 300001):
  _standardize(_count)


@case('vtc_extract_patches', 'all-four-borders', 'patches at every image edge')
def _extract(lib):
  count, h, w, c, ph, pw = 3, 21, 30, 2, 8, 5
  rs = np.random.RandomState(4)
  imgs = rs.randn(count, h, w, c).astype(np.float32)
  corners = [(0, 0), (0, w - pw), (h - ph, 0), (h - ph, w - pw), (0, 11),
             (h - ph, 11), (6, 0), (6, w - pw), (5, 9)]
  idx = np.array([i % count for i in range(len(corners))], np.int32)
  vert = np.array([v for v, _ in corners], np.int32)
  horz = np.array([u for _, u in corners], np.int32)
  num = len(corners)

  def call(lib, p, ws, wsb, st):
    return lib.vtc_extract_patches(p['imgs'], p['idx'], p['vert'], p['horz'],
                                   p['out'], num, h, w, c, ph, pw, st)

  def truth(want, inp):
    ref = np.stack([imgs[idx[i], vert[i]:vert[i] + ph,
                         horz[i]:horz[i] + pw, :].reshape(-1)
                    for i in range(num)])
    return [_exact('patches', want['out'], ref)]
  return Spec({'imgs': imgs, 'idx': idx, 'vert': vert, 'horz': horz},
              {'out': ((num, ph * pw * c), np.float32)}, call, truth)


# ------------------------------------------------------------------ ZCA / PCA
def _covariance(name, rows, cols, center, want_means, want_grand, want_cov):
  @case('vtc_column_covariance', name, 'row slabs in the workspace')
  def make(lib):
    x = (np.random.RandomState(rows + cols).randn(rows, cols) + 0.5).astype(
        np.float32)
    need = lib.vtc_column_covariance_workspace_bytes(rows, cols)
    outs = {'means': ((cols,), np.float64) if want_means else None,
            'grand': ((1,), np.float64) if want_grand else None,
            'cov': ((cols, cols), np.float64) if want_cov else None}

    def call(lib, p, ws, wsb, st):
      return lib.vtc_column_covariance(p['x'], rows, cols, center,
                                       p['means'], p['grand'], p['cov'], ws,
                                       wsb, st)

    def truth(want, inp):
      x64 = x.astype(np.float64)
      mu = x64.mean(0)
      xc = x64 - mu if center else x64
      out = []
      # tests/test_zca_gpu.py: float64 sums, 1e-9 / 1e-12
      if want_cov:
        ref = xc.T @ xc / rows
        out.append(('cov', float(np.linalg.norm(want['cov'] - ref) /
                                 np.linalg.norm(ref)), 1e-9))
        out.append(_exact('cov symmetric', want['cov'], want['cov'].T))
      if want_means:
        out.append(('means', float(np.abs(want['means'] - mu).max()), 1e-12))
      if want_grand:
        out.append(('grand mean', abs(float(want['grand'][0]) - mu.mean()),
                    1e-12))
      return out
    return Spec({'x': x}, outs, call, truth, ws_bytes=need, tight=True)
  return make


_covariance('all-outputs', 1000, 97, 1, True, True, True)
_covariance('cov-only-centered', 333, 64, 1, False, False, True)
_covariance('cov-only-uncentered', 333, 64, 0, False, False, True)
_covariance('means-only', 333, 65, 0, True, False, False)
_covariance('grand-only', 333, 65, 0, False, True, False)
_covariance('cov-and-means', 333, 64, 1, True, False, True)
_covariance('cov-and-grand', 333, 64, 1, False, True, True)
_covariance('means-and-grand', 333, 65, 0, True, True, False)
_covariance('means-and-cov-one-row', 1, 5, 0, True, False, True)


def _sym_eig(n):
  @case('vtc_sym_eig', 'n%d' % n, 'one workgroup Jacobi, float64 scratch')
  def make(lib):
    rs = np.random.RandomState(n)
    q, _ = np.linalg.qr(rs.randn(n, n))
    w = np.sort(rs.rand(n) + 0.1)[::-1] * np.linspace(1, 3, n)[::-1]
    a = (q * w) @ q.T
    a = (a + a.T) / 2
    need = lib.vtc_sym_eig_workspace_bytes(n)

    def call(lib, p, ws, wsb, st):
      return lib.vtc_sym_eig(p['a'], n, 30, p['w'], p['v'], p['status'], ws,
                             wsb, st)

    def truth(want, inp):
      assert int(want['status'][0]) == 1
      ref = np.linalg.eigvalsh(a)[::-1]
      v = want['v'].astype(np.float64)
      norm2 = np.abs(ref).max()
      # the gates of tests/test_zca_gpu.py
      return [('eigenvalues', float(np.abs(want['w'] - ref).max() / norm2),
               1e-6),
              ('residual', float(np.linalg.norm(a @ v - v * want['w'][None]) /
                                 np.linalg.norm(a)), 2e-6),
              ('orthogonality', float(np.abs(v.T @ v - np.eye(n)).max()),
               2e-6)]
    return Spec({'a': a}, {'w': ((n,), np.float64),
                           'v': ((n, n), np.float32),
                           'status': ((2,), np.int32)}, call, truth,
                ws_bytes=need, tight=True)
  return make


for _n in (1, 17, 256):
  _sym_eig(_n)


def _zca_matrices(n, null):
  @case('vtc_zca_matrices', 'n%d-null-%s' % (n, null or 'none'),
        'float64 sums, n x n outputs')
  def make(lib):
    rs = np.random.RandomState(n + 7)
    u, _ = np.linalg.qr(rs.randn(n, n))
    u = u.astype(np.float32)
    w = np.sort(rs.rand(n))[::-1].copy()
    w[-1] = -1e-9                       # negative eigenvalues count as 0
    eps = 1e-4
    outs = {'w': None if null == 'w' else ((n, n), np.float32),
            'winv': None if null == 'winv' else ((n, n), np.float32)}

    def call(lib, p, ws, wsb, st):
      return lib.vtc_zca_matrices(p['u'], p['vals'], n, eps, p['w'],
                                  p['winv'], st)

    def truth(want, inp):
      u64 = u.astype(np.float64)
      root = np.sqrt(np.maximum(w, 0)) + eps
      out = []
      for key, diag in (('w', 1 / root), ('winv', root)):
        if outs[key] is None:
          continue
        ref = (u64 * diag) @ u64.T
        # float64 sum of n terms rounded once to float32
        mag = (np.abs(u64) * diag) @ np.abs(u64).T
        out.append(_elementwise(key, want[key], ref,
                                U24 * np.abs(ref) + n * 2.0 ** -53 * mag))
      return out
    return Spec({'u': u, 'vals': w}, outs, call, truth)
  return make


for _n, _null in ((1, None), (97, None), (97, 'w'), (97, 'winv'),
                  (260, None)):
  _zca_matrices(_n, _null)


def _row_transform(n, rows):
  @case('vtc_row_transform', 'n%d-rows%d' % (n, rows),
        'float32 FMA chains in k order')
  def make(lib):
    rs = np.random.RandomState(n + rows)
    x = rs.randn(rows, n).astype(np.float32)
    off = rs.randn(n).astype(np.float32)
    m = (rs.randn(n, n) / np.sqrt(n)).astype(np.float32)
    add = 0.25

    def call(lib, p, ws, wsb, st):
      return lib.vtc_row_transform(p['x'], rows, n, p['off'], p['m'], add,
                                   p['y'], st)

    def truth(want, inp):
      xc = (x - off[None, :]).astype(np.float64)   # float32 centring
      m64 = m.astype(np.float64)
      ref = xc @ m64 + add
      mag = np.abs(xc) @ np.abs(m64) + abs(add)
      return [_elementwise('y', want['y'], ref, (n + 1) * U24 * mag)]
    return Spec({'x': x, 'off': off, 'm': m}, {'y': ((rows, n), np.float32)},
                call, truth)
  return make


for _n in (3, 256, 260, 1024):
  for _rows in (1, 1000):
    _row_transform(_n, _rows)


def _mat_inverse(n):
  @case('vtc_mat_inverse', 'n%d' % n, 'float64 LU in the workspace')
  def make(lib):
    import ica_data
    a = ica_data.conditioned(n, 1e2, 12 + n)
    need = lib.vtc_mat_inverse_workspace_bytes(n)

    def call(lib, p, ws, wsb, st):
      return lib.vtc_mat_inverse(p['a'], n, p['inv'], p['status'], ws, wsb,
                                 st)

    def truth(want, inp):
      assert want['status'].tolist() == [1, -1]
      import ica_data
      ref = np.linalg.inv(a.astype(np.float64))
      return [('inverse', ica_data.rel(want['inv'], ref), 1e-6)]
    return Spec({'a': a}, {'inv': ((n, n), np.float32),
                           'status': ((2,), np.int32)}, call, truth,
                ws_bytes=need, tight=True)
  return make


for _n in (1, 5, 64, 256):
  _mat_inverse(_n)


# -------------------------------------------------------- local normalisation
def _gauss_symm(x, sigma):
  """get_gaussian_filter_2d(sigma, (4 sigma + 1,) * 2) applied per channel as
  two 1D float64 passes, 'same' size, scipy's 'symm' boundary."""
  radius = int(2 * sigma)
  t = np.arange(-radius, radius + 1, dtype=np.float64)
  g = np.exp(-t ** 2 / (2.0 * sigma ** 2))
  g /= g.sum()

  def conv_axis(a, axis):
    size = a.shape[axis]
    idx = np.arange(-radius, size + radius)
    period = 2 * size
    idx = np.mod(idx, period)
    idx = np.where(idx >= size, period - 1 - idx, idx)
    padded = np.take(a, idx, axis=axis)
    out = np.zeros_like(a)
    for k in range(2 * radius + 1):
      sl = [slice(None)] * a.ndim
      sl[axis] = slice(k, k + size)
      out += g[2 * radius - k] * padded[tuple(sl)]
    return out
  return conv_axis(conv_axis(x.astype(np.float64), 1), 2)


def _local_normalize(name, h, w, c, sigma, mode, count=2):
  @case('vtc_local_normalize', name, 'LDS tiles, NULL workspace'
        if 2 * sigma <= 16 else 'float64 planes in the workspace')
  def make(lib):
    x = np.random.RandomState(h * w + int(sigma)).rand(count, h, w, c).astype(
        np.float32) + np.float32(0.1)
    need = lib.vtc_local_normalize_workspace_bytes(count, h, w, c, sigma)

    def call(lib, p, ws, wsb, st):
      return lib.vtc_local_normalize(p['x'], p['out'], p['aux'], count, h, w,
                                     c, sigma, mode, ws, wsb, st)

    def truth(want, inp):
      x64 = x.astype(np.float64)
      if mode == 0:
        aux = _gauss_symm(x, sigma)
        ref = x64 - aux
      else:
        v = _gauss_symm(x * x, sigma)
        aux = np.sqrt(np.where(v == 0, 1.0, v))
        ref = x64 / aux
      # float64 filter rounded to float32, then a float32 epilogue: the
      # figure tests/test_dataset_gpu.py holds these ops to
      return [('aux', helpers.rel_err(want['aux'], aux), 1e-6),
              ('out', helpers.rel_err(want['out'], ref), 1e-5)]

    def route(lib):
      assert (need == 0) == (2 * sigma <= 16)
    return Spec({'x': x}, {'out': (x.shape, np.float32),
                           'aux': (x.shape, np.float32)}, call, truth,
                ws_bytes=need, tight=need > 0, route=route)
  return make


for _mode in (0, 1):
  _local_normalize('sigma2-mode%d-37x53x3' % _mode, 37, 53, 3, 2.0, _mode)
  _local_normalize('sigma2-mode%d-5x7x2-smaller-than-window' % _mode, 5, 7, 2,
                   2.0, _mode)
  _local_normalize('sigma9-mode%d-37x53x3' % _mode, 37, 53, 3, 9.0, _mode)
  _local_normalize('sigma9-mode%d-20x11x1-smaller-than-window' % _mode, 20,
                   11, 1, 9.0, _mode)


def _patch_matrix(dtype, rows, cols):
  rs = np.random.RandomState(rows + cols)
  if dtype == 1:
    return rs.randint(0, 256, size=(rows, cols)).astype(np.uint8)
  return (rs.randn(rows, cols) + 0.3).astype(np.float32)


def _column_stats(dtype, cols, rows=301):
  tag = '%s-cols%d' % ('u8' if dtype else 'f32', cols)

  for null in (None, 'mean', 'var'):
    @case('vtc_column_moments', '%s-null-%s' % (tag, null or 'none'),
          'float64 row-slab partials in the workspace')
    def moments(lib, null=null):
      x = _patch_matrix(dtype, rows, cols)
      need = lib.vtc_column_moments_workspace_bytes(rows, cols)
      outs = {'mean': None if null == 'mean' else ((cols,), np.float32),
              'var': None if null == 'var' else ((cols,), np.float32)}

      def call(lib, p, ws, wsb, st):
        return lib.vtc_column_moments(p['x'], dtype, rows, cols, p['mean'],
                                      p['var'], ws, wsb, st)

      def truth(want, inp):
        x64 = x.astype(np.float64)
        out = []
        # float64 sums rounded once: tests/test_dataset_gpu.py figures
        if null != 'mean':
          out.append(('mean', helpers.rel_err(want['mean'], x64.mean(0)),
                      1e-7))
        if null != 'var':
          out.append(('var', helpers.rel_err(want['var'], x64.var(0)), 1e-6))
        return out
      return Spec({'x': x}, outs, call, truth, ws_bytes=need, tight=need > 0)

  for op in (0, 1):
    @case('vtc_column_apply', '%s-op%d' % (tag, op), 'element-wise')
    def apply_(lib, op=op):
      x = _patch_matrix(dtype, rows, cols)
      v = (0.5 + np.random.RandomState(cols).rand(cols)).astype(np.float32)

      def call(lib, p, ws, wsb, st):
        return lib.vtc_column_apply(p['x'], dtype, rows, cols, op, p['v'],
                                    p['out'], st)

      def truth(want, inp):
        xf = x.astype(np.float32)
        if op == 0:
          return [_exact('x - v', want['out'], xf - v[None, :])]
        ref = xf.astype(np.float64) / np.sqrt(v.astype(np.float64))[None, :]
        # a float32 square root and a float32 division
        return [_elementwise('x / sqrt(v)', want['out'], ref,
                             3 * U24 * np.abs(ref))]
      return Spec({'x': x, 'v': v}, {'out': ((rows, cols), np.float32)}, call,
                  truth)

  for with_means in (True, False):
    @case('vtc_row_center', '%s-means%d' % (tag, with_means),
          'float64 row sums')
    def center(lib, with_means=with_means):
      x = _patch_matrix(dtype, 33, cols)
      outs = {'out': ((33, cols), np.float32),
              'means': ((33,), np.float32) if with_means else None}

      def call(lib, p, ws, wsb, st):
        return lib.vtc_row_center(p['x'], dtype, 33, cols, p['out'],
                                  p['means'], st)

      def truth(want, inp):
        x64 = x.astype(np.float64)
        mu = x64.mean(1)
        # the mean: a float64 sum of `cols` terms rounded once to float32;
        # the output: that rounding and one float32 subtraction
        mu_bound = U24 * np.abs(mu) + cols * 2.0 ** -53 * np.abs(x64).mean(1)
        ref = x64 - mu[:, None]
        out = [_elementwise('x - mean', want['out'], ref,
                            U24 * np.abs(ref) + mu_bound[:, None] + TINY)]
        if with_means:
          out.append(_elementwise('means', want['means'], mu,
                                  mu_bound + TINY))
        return out
      return Spec({'x': x}, outs, call, truth)


for _dtype in (0, 1):
  for _cols in (1, 64, 97):
    _column_stats(_dtype, _cols)


@pytest.mark.parametrize('c', CASES, ids=[c.id for c in CASES])
def test_fenced_call(device, c):
  run_case(device, c)
