"""The two MFMA tiles of the fused FISTA kernel (csrc/fc_fused.hip): the same
32x32 output tile per wave from 32x32x16 or from 16x16x32 instructions, which
have different lane maps.  VTC_FUSED_TILE=32|16 forces one; the library reads
it on every call."""
import ctypes

import numpy as np
import pytest
import torch

import fences
import helpers
import sc_oracle

pytestmark = pytest.mark.gpu

TILES = ('32', '16')
REL_TOL_BF16 = 5e-2     # the gate of test_fc_fused_gpu.py's bf16 fast mode
SPLIT = {'f16x3': (helpers.REL_TOL_F32, helpers.REL_TOL_SHORT,
                   helpers.NEAR_THRESHOLD),
         'bf16x3': (helpers.REL_TOL_BF16X3, 1e-5, 5e-6)}


@pytest.fixture(scope='module')
def ista_fista():
  from analysis_transforms.fully_connected import ista_fista
  if not ista_fista.fused_available():
    pytest.fail('libvtc_hip.so was built without the fused FISTA kernel')
  return ista_fista


@pytest.fixture
def tile(monkeypatch):
  def force(which):
    monkeypatch.setenv('VTC_FUSED_TILE', which)
  return force


def _c2(device):
  g = helpers.load('fc_c2_mini')
  X = helpers.to_dev(helpers.gaussian_patches(0, 64, 256), device)
  D = helpers.to_dev(helpers.unit_rows(1, 1024, 256), device)
  return g, X, D, float(g['sparsity_weight']), float(g['stepsize'])


# ------------------------------------------------------------ 1. index maps
ETA = 2.0 ** -4          # stepsize, a power of two
LAM = 4.0                # lambda * eta = 1/4


def _integer_inputs(b, s):
  a = np.arange(s)[:, None]
  p = np.arange(256)[None, :]
  i = np.arange(b)[:, None]
  D = ((7 * a + 3 * p) % 5 - 2).astype(np.float32)   # not normalised
  X = ((i + 2 * p) % 7 - 3).astype(np.float32)
  return X, D


def _granule(x):
  """The largest power of two that divides every entry of x."""
  x = x[x != 0]
  if x.size == 0:
    return 1.0
  u = 2.0 ** np.floor(np.log2(np.abs(x).max()))
  while not np.all(np.mod(x / u, 1) == 0):
    u /= 2
  return u


def _assert_exact_product(A, B, operand_bits, what):
  """A @ B on split operands is exact: every entry of the streamed operand A
  fits `operand_bits` significant bits, B (the dictionary) fits the hi part
  alone, so the dropped lo*lo product is zero, and every sum of |terms| stays
  below 2^24 granules, so any f32 summation order gives the same bits."""
  ua, ub = _granule(A), _granule(B)
  assert np.abs(A).max() / ua < 2.0 ** operand_bits, what
  assert np.abs(B).max() / ub < 2.0 ** 8, what
  assert (np.abs(A) @ np.abs(B)).max() / (ua * ub) < 2.0 ** 24, what


def _assert_f32(x, what):
  assert np.array_equal(x, x.astype(np.float32).astype(np.float64)), what


def _restate_float64(X, D, iters, fista, init, operand_bits):
  """The iteration in float64, asserting on the way that every operand of both
  products and every intermediate is exact in the kernel's formats.  Only
  momentum-free runs are exact: ISTA, or FISTA's first iteration (beta_1 = 0)."""
  assert not fista or iters == 1
  X, D = X.astype(np.float64), D.astype(np.float64)
  cut = LAM * ETA
  y = np.zeros((X.shape[0], D.shape[0])) if init is None else init.astype(
      np.float64)
  for k in range(iters):
    if np.any(y):
      _assert_exact_product(y, D, operand_bits, 'Y D, iteration %d' % k)
    r = y @ D - X
    _assert_f32(r, 'residual')
    _assert_exact_product(r, D.T, operand_bits, 'R D^T, iteration %d' % k)
    g = r @ D.T
    c = y - ETA * g
    for v, name in ((g, 'gradient'), (c, 'gradient step')):
      _assert_f32(v, name)
    y = np.sign(c) * np.maximum(np.abs(c) - cut, 0)
    _assert_f32(y, 'codes')
  return y


INDEX_RUNS = [('fista', 1, False), ('ista', 1, False), ('ista', 2, False),
              ('fista', 1, True)]


@pytest.mark.parametrize('s', [256, 512, 1024])
def test_index_maps_exactly(device, ista_fista, tile, s):
  """Integer-valued inputs free of symmetry, a power-of-two stepsize and a
  dyadic threshold: every product and sum of the run is exact in f32, so the
  codes equal the oracle's bit for bit whatever the summation order -- and any
  mistake in a lane map, which tolerance tests on random data can miss, shows.
  All three phase counts, partial workgroups with both patch halves of a lane
  partly dead, both tiles.  f16x3 (22-bit operands) and bf16x3 (16-bit) run
  every case, ISTA T = 2 included (exact at these magnitudes: operands stay
  below 14 bits, sums below 22); bf16 (8 bits) the cold T = 1 cases."""
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
        for which in TILES:
          tile(which)
          out = ista_fista.run(
              X, D, LAM, iters, variant=variant, precision=prec, stepsize=ETA,
              initial_codes=None if init is None else helpers.to_dev(
                  init, device))
          assert torch.equal(out.cpu(), ref), (b, variant, iters, warm_start,
                                               prec, which)


# ------------------------------------------------ 2. parity of the forced arm
@pytest.mark.parametrize('prec', ['f16x3', 'bf16x3'])
@pytest.mark.parametrize('other', TILES)
def test_forced_tile_matches_reference_trace(device, ista_fista, tile, other,
                                             prec):
  """The cases of test_fc_fused_gpu.py through each tile by force -- whichever
  of them is not the default of the precision included -- at the same
  tolerances."""
  tile(other)
  g, X, D, lam, eta = _c2(device)
  long_tol, short_tol, flip = SPLIT[prec]
  for k, tol in ((1, short_tol), (2, short_tol), (20, short_tol),
                 (200, long_tol)):
    codes = ista_fista.run(X, D, lam, k, precision=prec, stepsize=eta)
    err, flips = helpers.assert_codes_match(
        codes.cpu().numpy(), g['codes_fista_T%d' % k], tol,
        '%s T=%d' % (prec, k), max_flip_mag=flip)
    print('tile %s fc_c2 %s T=%d rel %.2e flips %d' % (other, prec, k, err,
                                                      flips))
  codes = ista_fista.run(X, D, lam, 50, variant='ista', precision=prec,
                         stepsize=eta)
  err, _ = helpers.assert_codes_match(
      codes.cpu().numpy(), g['codes_ista_T50'], short_tol, prec + ' ista',
      max_flip_mag=flip)
  print('tile %s fc_c2 %s ista T=50 rel %.2e' % (other, prec, err))
  init = helpers.to_dev(g['codes_fista_T20'], device)
  keep = init.clone()
  warm = ista_fista.run(X, D, lam, 20, precision=prec, stepsize=eta,
                        initial_codes=init)
  assert torch.equal(init, keep)
  err, _ = helpers.assert_codes_match(
      warm.cpu().numpy(), g['codes_fista_warm20'], short_tol,
      prec + ' warm start', max_flip_mag=flip)
  print('tile %s fc_c2 %s warm start rel %.2e' % (other, prec, err))
  w = helpers.load('whitened')
  Xw = helpers.to_dev(w['images'], device)
  Dw = helpers.to_dev(helpers.unit_rows(int(w['seed_dictionary']), 512, 256),
                      device)
  codes = ista_fista.run(Xw, Dw, float(w['sparsity_weight']), 100,
                         precision=prec, stepsize=float(w['stepsize']))
  err, _ = helpers.assert_codes_match(
      codes.cpu().numpy(), w['codes_fista_T100'], long_tol,
      prec + ' whitened (s=512)', max_flip_mag=5e-6)
  print('tile %s whitened %s T=100 rel %.2e' % (other, prec, err))


@pytest.mark.parametrize('other', TILES)
def test_forced_tile_bf16_fast_mode(device, ista_fista, tile, other):
  tile(other)
  g, X, D, lam, eta = _c2(device)
  codes = ista_fista.run(X, D, lam, 200, precision='bf16', stepsize=eta)
  err = helpers.rel_err(codes.cpu().numpy(), g['codes_fista_T200'])
  print('tile %s fc_c2 bf16 T=200 rel %.2e' % (other, err))
  assert err < REL_TOL_BF16
  one = ista_fista.run(X, D, lam, 1, precision='bf16', stepsize=eta)
  assert helpers.rel_err(one.cpu().numpy(), g['codes_fista_T1']) < 2e-2


# --------------------------------------------------- 3. f16x3 scale invariance
@pytest.mark.parametrize('other', TILES)
def test_forced_tile_f16x3_scale_invariance(device, ista_fista, tile, other):
  """Patches and lambda times 2^k give codes times 2^k bit for bit.  A lane of
  the 16x16x32 kernel owns two patches: in the mixed batch the two patches of
  every lane (rows i and 16 + i of a workgroup) differ by 2^20, so a per-patch
  scalar applied to the wrong one of them cannot pass."""
  tile(other)
  g, X, D, lam, eta = _c2(device)
  base = ista_fista.run(X, D, lam, 30, precision='f16x3', stepsize=eta)
  for k in (-40, 9, 40):
    f = float(2.0 ** k)
    out = ista_fista.run(X * f, D, lam * f, 30, precision='f16x3',
                         stepsize=eta)
    assert torch.equal(out, base * f), k
  # rows 16..31 and 48..63 (the second patch of every lane) times 2^20, and
  # one row of each half on a scale of its own; lambda scales per row, so run
  # each scale group with its own lambda and compare rows
  scale = torch.ones(64, device=X.device)
  scale[16:32] = float(2.0 ** 20)
  scale[48:64] = float(2.0 ** 20)
  scale[5] = float(2.0 ** -13)
  scale[21] = float(2.0 ** 7)
  mixed = X * scale[:, None]
  for f in (1.0, 2.0 ** 20, 2.0 ** -13, 2.0 ** 7):
    rows = scale == f
    out = ista_fista.run(mixed, D, lam * f, 30, precision='f16x3',
                         stepsize=eta)
    assert torch.equal(out[rows], base[rows] * f), f


# ----------------------------------------------------------- 4. ragged batch
def _fenced_run(device, X, D, lam, eta, iters, prec):
  """vtc_fc_ista_fista with the codes inside a guard band."""
  import vtc_hip
  lib = vtc_hip.load_library()
  b, n = X.shape
  s = D.shape[0]
  code = vtc_hip.PRECISIONS[prec]
  ws = vtc_hip.workspace(lib.vtc_fc_ista_fista_workspace_bytes(b, n, s, code),
                         device)
  codes, fence = fences.fenced((b, s), torch.float32, device)
  done = ctypes.c_int(0)
  status = lib.vtc_fc_ista_fista(
      vtc_hip.ptr(X), vtc_hip.ptr(D), vtc_hip.ptr(None), vtc_hip.ptr(codes),
      b, n, s, float(eta), float(lam), int(iters),
      vtc_hip.variant_code('fista'), vtc_hip.threshold_mode(False, False),
      -1.0, code, vtc_hip.ptr(ws), ws.numel(), ctypes.byref(done),
      vtc_hip.current_stream(device))
  vtc_hip.check(status, 'vtc_fc_ista_fista')
  fence.assert_intact('codes of b = %d' % b)
  fence.assert_written('codes of b = %d' % b)
  return codes.clone()


@pytest.mark.parametrize('prec', ['f16x3', 'bf16x3'])
@pytest.mark.parametrize('which', TILES)
def test_ragged_batch_rows_are_independent(device, ista_fista, tile, which,
                                           prec):
  """b = 70 against its first 64 and last 6 rows run separately: bit-equal
  rows (nothing leaks between patches through the LDS exchange images), and
  no row past b is written (guard band around the codes)."""
  tile(which)
  X = helpers.to_dev(helpers.gaussian_patches(770, 70, 256), device)
  D = helpers.to_dev(helpers.unit_rows(771, 512, 256), device)
  full = _fenced_run(device, X, D, 0.02, 0.2, 12, prec)
  head = _fenced_run(device, X[:64].contiguous(), D, 0.02, 0.2, 12, prec)
  tail = _fenced_run(device, X[64:].contiguous(), D, 0.02, 0.2, 12, prec)
  assert torch.equal(full[:64], head)
  assert torch.equal(full[64:], tail)
  assert float(full.abs().max()) > 0
