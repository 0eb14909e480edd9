"""One large batch per fully-connected and convolutional inference route that
the other large-batch tests do not cover (fc_small, fc_chip16, the tiled
run_generic path in f32 and f16x3 -- with and without a split-K residual --,
the streamed kernel's FC form, and the three exact-f32 conv routes: patch
contractions, stride-1 direct kernels, general direct kernels): enough
workgroups to keep every CU busy for several rounds, two runs bit-identical,
and a seeded sample of rows against the float64 oracle on the CPU.

A store hazard that corrupted ~0.03 % of the codes only at large batches
(csrc/epi_prox.h) passed every small test; these cases are sized so that such
a fault shows up in the sample and in the run-to-run comparison."""
import ctypes

import numpy as np
import pytest
import torch

import conv_routes_data as crd
import helpers
import sc_oracle

pytestmark = pytest.mark.gpu

SAMPLE = 2048


@pytest.fixture(scope='module')
def fc():
  from analysis_transforms.fully_connected import ista_fista
  return ista_fista


def _patches(device, seed, b, n):
  gen = torch.Generator(device=device)
  gen.manual_seed(seed)
  return 0.1 * torch.randn(b, n, device=device, generator=gen)


def _sample(seed, b, count=SAMPLE):
  rows = np.random.RandomState(seed).choice(b, size=min(count, b),
                                            replace=False)
  rows.sort()
  return rows


def _x3_want_slices(M, N, K):
  """gemm_x3_want_slices (csrc/gemm_x3.h): K slices of a split-precision
  product with few 128 x 128 output tiles."""
  ceil = lambda a, b: -(-a // b)
  want = min(ceil(512, ceil(M, 128) * ceil(N, 128)), ceil(K, 256), 16)
  want = max(want, 1)
  chunk = max(ceil(ceil(K, want), 32) * 32, 32)
  return ceil(K, chunk)


# (name, n, s, b, variant, precision passed, route the policy must pick)
FC_CASES = [
    ('fc_small s=64', 64, 64, 1 << 20, 'ista', None, 'f32'),
    ('fc_small s=192', 64, 192, 1 << 20, 'ista', None, 'f32'),
    ('fc_chip16', 144, 576, 1 << 17, 'fista', None, 'f32'),
    ('generic f32', 100, 200, 1 << 17, 'fista', 'f32', None),
    ('generic f16x3', 100, 200, 1 << 17, 'fista', None, 'f16x3'),
    ('generic f16x3 split-K', 100, 2400, 8192, 'fista', None, 'f16x3'),
    ('streamed fc', 256, 2048, 1 << 15, 'fista', None, 'f16x3'),
]


@pytest.mark.parametrize('case', FC_CASES, ids=[c[0] for c in FC_CASES])
def test_fully_connected_route(device, fc, case):
  """8x8 patches against 64 / 192 atoms take csrc/fc_small.hip, 12x12
  against 576 csrc/fc_chip16.hip (both only for exact f32, which 'auto'
  picks there); n = 100 is none of the on-chip shapes, so f32 runs the tiled
  exact-f32 path of run_generic (fc_inference.hip; ragged 32-wide tiles:
  100 and 200 are not multiples of 32) and 'auto' the tiled f16 split, whose
  residual product splits its K axis when the batch gives few output tiles;
  16x16 patches against 2048 atoms take the streamed kernel
  (csrc/fused_stream.hip).  T = 20, tolerance 5e-6 against float64, flips
  only within 2e-6 of the threshold."""
  import vtc_hip
  name, n, s, b, variant, precision, policy = case
  if policy is not None:
    assert fc._resolve_precision(None, b, n, s, None) == (
        vtc_hip.PRECISIONS[policy])
  if name.startswith('generic'):
    assert n not in (64, 144, 256)
  if name.endswith('split-K'):
    assert _x3_want_slices(b, n, s) > 1
  elif name.startswith('generic'):
    assert _x3_want_slices(b, n, s) == 1
  if name == 'streamed fc':
    assert s not in (256, 512, 1024)          # not a shape of the fused kernel
  lam, iters = 0.02, 20
  X = _patches(device, 1000 + s, b, n)
  Dn = helpers.unit_rows(2000 + s, s, n)
  D = helpers.to_dev(Dn, device)
  eta = float(sc_oracle.fc_stepsize(torch.from_numpy(Dn)))
  first = fc.run(X, D, lam, iters, variant=variant, precision=precision,
                 stepsize=eta)
  again = fc.run(X, D, lam, iters, variant=variant, precision=precision,
                 stepsize=eta)
  assert torch.equal(first, again), name + ': runs differ'
  if name == 'streamed fc':
    # early stopping that never fires (mean < 0) keeps the same f16x3 split
    # but bypasses the streamed kernel: the tiled path.  A default run that
    # differs from it is not on the tiled path; with no fused shape left, it
    # ran on the streamed kernel.
    tiled = fc.run(X, D, lam, iters, variant=variant, precision='f16x3',
                   stepsize=eta, early_stopping_epsilon=0.0)
    assert fc.run.last_iters == iters
    assert not torch.equal(first, tiled)
    del tiled
  rows = torch.from_numpy(_sample(3000 + s, b)).to(device)
  Xs = X[rows].double().cpu()
  ref = sc_oracle.fc_ista_fista(Xs, torch.from_numpy(Dn).double(), lam, iters,
                                variant=variant, stepsize=eta)
  ours = first[rows].cpu().numpy()
  err, flips = helpers.assert_codes_match(
      ours, ref.numpy(), helpers.REL_TOL_SHORT, name,
      max_flip_mag=helpers.NEAR_THRESHOLD)
  print('%-24s b=%d rel %.2e vs float64, %d flips' % (name, b, err, flips))


def _conv_route(geom):
  """Which exact-f32 route vtc_conv_ista_fista takes for a geometry: the
  family of the dispatch mirror in tests/conv_routes_data.py (patch, unit,
  or direct -- the direct analysis behind either synthesis)."""
  family = crd.conv_route(geom, 'f32', torch.cuda.get_device_properties(
      0).multi_processor_count)[0]
  return 'direct' if family == 'unit-synth+direct' else family


# (name, stride, kernel size, kernels, image size, images, precision passed,
#  exact-f32 route)
CONV_CASES = [
    # im2col + exact-f32 MFMA contractions (csrc/conv_patch.h)
    ('patch k=8 stride 4', 4, 8, 32, 256, 16, None, 'patch'),
    # scalar-tap direct kernels of stride-1 square kernels (csrc/conv_unit.h);
    # 'auto' would take the f16x3 matrix-core route here
    ('unit k=11 stride 1', 1, 11, 32, 128, 16, 'f32', 'unit'),
    # general direct kernels (conv_synth_residual_kernel,
    # conv_analysis_prox_kernel): each pixel under 8 x 8 code positions is
    # beyond the patch route's 16
    ('direct k=16 stride 2', 2, 16, 32, 128, 64, None, 'direct'),
]


@pytest.mark.parametrize('case', CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_exact_f32_conv_route(device, case):
  """The three exact-f32 convolution routes on large batches.  Strided
  geometries have no split-precision form, so 'auto' runs exact f32 there;
  stride 1 asks for it.  FISTA T = 20 at eta = 1 / (cover * lambda_max(F F^T)),
  cover = code positions over a pixel, a bound on the operator norm, so the
  iterates converge.  Two runs bit-identical; 4 of the images against the
  float64 oracle at 5e-6, flips only within 2e-6 of the threshold."""
  import vtc_hip
  from analysis_transforms.convolutional import ista_fista as conv
  from utils import convolutions
  name, stride, k, s, size, b, precision, route = case
  lead, trail = sc_oracle.conv_padding_amount(size, k, stride)
  rs = np.random.RandomState(4000 + k)
  imgs = np.zeros((b, 1, size + lead + trail, size + lead + trail),
                  np.float32)
  imgs[:, :, lead:lead + size, lead:lead + size] = (
      0.5 * rs.randn(b, 1, size, size)).astype(np.float32)
  Dn = rs.randn(s, 1, k, k).astype(np.float32)
  Dn /= np.sqrt((Dn.astype(np.float64) ** 2).sum(axis=(1, 2, 3)))[
      :, None, None, None].astype(np.float32)
  pad = ((lead, trail), (lead, trail))
  strides = (stride, stride)
  X, D = helpers.to_dev(imgs, device), helpers.to_dev(Dn, device)
  geom = convolutions.geometry(X, D, strides, pad)
  assert _conv_route(geom) == route
  x3 = vtc_hip.load_library().vtc_conv_x3_supported(ctypes.byref(geom))
  assert bool(x3) == (stride == 1)
  assert precision == 'f32' or not x3
  cover = (-(-k // stride)) ** 2
  eta = float(sc_oracle.conv_stepsize(torch.from_numpy(Dn))) / cover
  lam, iters = 0.05, 20
  first = conv.run(X, D, strides, pad, lam, iters, stepsize=eta,
                   precision=precision)
  again = conv.run(X, D, strides, pad, lam, iters, stepsize=eta,
                   precision=precision)
  assert torch.equal(first, again), name + ': runs differ'
  pick = _sample(4001 + k, b, 4)
  ref = sc_oracle.conv_ista_fista(torch.from_numpy(imgs[pick]).double(),
                                  torch.from_numpy(Dn).double(), strides, pad,
                                  lam, iters, stepsize=eta)
  ours = first[torch.from_numpy(pick).to(device)].cpu().numpy()
  err, flips = helpers.assert_codes_match(
      ours, ref.numpy(), helpers.REL_TOL_SHORT, name,
      max_flip_mag=helpers.NEAR_THRESHOLD)
  print('%-24s b=%d rel %.2e vs float64, %d flips, %.1f %% non-zero' % (
      name, b, err, flips, 100.0 * float((ref != 0).double().mean())))
