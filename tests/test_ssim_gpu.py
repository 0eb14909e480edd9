"""utils.plotting.compute_ssim / compute_ssim_images (csrc/ssim.hip) against
float64 truth: tests/golden/ssim.npz, written with scipy's gaussian_filter,
for the float32 pairs, and the numpy restatement tests/ssim_oracle.py (held to
that fixture by tests/test_ssim_host.py) for float64 pairs made here.

The bound is 1e-9 absolute on maps and means, derived in DESIGN.md 4.13: an
11-tap float64 sum applied twice leaves each moment within about 2.4e-15 M^2,
M = max(|x|, |y|); each of the four factors of S is at least C1 = 1e-4 R^2;
with M <= 2 R every factor is within 1e-10 relative and |S| <= 1, so the map
is within about 2e-10.  Every input here keeps M <= 2 R (asserted).

Shapes (16 x 32 is the kernel's output tile, pinned by the workspace query in
tests/test_ssim_host.py): 11x11, 12x17, 16x32, 17x33, 37x131, 11x300, 300x11;
data of range 1, of range 255, zero-centred, and a constant image with one
outlier pixel against the same image with the outlier elsewhere.
"""
import numpy as np
import pytest
import torch

import helpers
import ssim_oracle

pytestmark = pytest.mark.gpu

BOUND = 1e-9
SWAP_BOUND = 1e-12
GOLDEN = helpers.load('ssim')
CASES = [str(c) for c in GOLDEN['cases']]


def _pair(tag):
  return (GOLDEN[tag + '_x'], GOLDEN[tag + '_y'],
          float(GOLDEN[tag + '_range']))


def _f64_pair(tag):
  """The pair as genuine float64 data: every sample shrunk by a factor in
  (1 - 2^-30, 1], so that it is no float32 number and M <= 2 R still holds."""
  x, y, r = _pair(tag)
  rs = np.random.RandomState(len(tag) + x.size)
  x64 = x.astype(np.float64) * (1. - rs.rand(*x.shape) * 2. ** -30)
  y64 = y.astype(np.float64) * (1. - rs.rand(*y.shape) * 2. ** -30)
  assert (x64.astype(np.float32).astype(np.float64) != x64).any()
  return x64, y64, r


def _run(device, x, y, ranges):
  """(means, maps) as numpy, of stacks or of one pair."""
  from utils import plotting
  single = x.ndim == 2
  xs, ys = (helpers.to_dev(a[None] if single else a, device) for a in (x, y))
  means, maps = plotting.compute_ssim_images(xs, ys, ranges, return_map=True)
  assert means.dtype == torch.float64 and maps.dtype == torch.float64
  assert means.shape == (xs.shape[0],) and maps.shape == xs.shape
  means, maps = means.cpu().numpy(), maps.cpu().numpy()
  return (means[0], maps[0]) if single else (means, maps)


def _assert_close(tag, mean, smap, want_mean, want_map):
  assert np.isfinite(smap).all(), tag
  gap_map = float(np.abs(smap - want_map).max())
  gap_mean = abs(float(mean) - float(want_mean))
  print('ssim %-22s map %.2e mean %.2e' % (tag, gap_map, gap_mean))
  assert gap_map <= BOUND, '%s: map off by %.3e' % (tag, gap_map)
  assert gap_mean <= BOUND, '%s: mean off by %.3e' % (tag, gap_mean)


@pytest.mark.parametrize('tag', CASES)
def test_float32_pairs_against_the_fixture(device, tag):
  from utils import plotting
  x, y, r = _pair(tag)
  assert max(np.abs(x).max(), np.abs(y).max()) <= 2 * r
  mean, smap = _run(device, x, y, r)
  _assert_close(tag, mean, smap, GOLDEN[tag + '_mean'], GOLDEN[tag + '_map'])
  # the reference's signature: a Python float, the same number
  single = plotting.compute_ssim(helpers.to_dev(x, device),
                                 helpers.to_dev(y, device), r)
  assert isinstance(single, float) and single == float(mean)


@pytest.mark.parametrize('tag', CASES)
def test_float64_pairs_against_the_restatement(device, tag):
  x, y, r = _f64_pair(tag)
  assert max(np.abs(x).max(), np.abs(y).max()) <= 2 * r
  want_mean, want_map = ssim_oracle.ssim(x, y, r)
  mean, smap = _run(device, x, y, r)
  _assert_close(tag + ' f64', mean, smap, want_mean, want_map)


@pytest.mark.parametrize('tag', CASES)
def test_own_range_is_the_float32_difference(device, tag):
  """manual_sig_mag=None: R is max - min of the float32 target formed in
  float32, then widened -- bitwise the call that is given that number."""
  from utils import plotting
  x, y, _ = _pair(tag)
  r_none = float(GOLDEN[tag + '_range_none'])
  assert r_none == float(x.max() - x.min())
  mean, smap = _run(device, x, y, None)
  given_mean, given_map = _run(device, x, y, r_none)
  assert mean == given_mean and np.array_equal(smap, given_map)
  assert abs(mean - float(GOLDEN[tag + '_mean_none'])) <= BOUND
  single = plotting.compute_ssim(helpers.to_dev(x, device),
                                 helpers.to_dev(y, device))
  assert single == float(mean)


def test_float32_difference_is_not_the_float64_one():
  """The convention can be told apart on this fixture."""
  apart = [tag for tag in CASES
           if float(GOLDEN[tag + '_x'].astype(np.float64).max() -
                    GOLDEN[tag + '_x'].astype(np.float64).min()) !=
           float(GOLDEN[tag + '_range_none'])]
  assert apart


def test_float64_targets_need_their_range(device):
  from utils import plotting
  x = torch.rand(12, 17, dtype=torch.float64, device=device)
  with pytest.raises(TypeError):
    plotting.compute_ssim(x, x)
  assert plotting.compute_ssim(x, x, 1.0) == 1.0


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_stack_of_three_equals_three_single_calls(device, dtype):
  tags = ['range1_12x17', 'range255_12x17', 'centred_12x17']
  pairs = [_pair(t) for t in tags]
  xs = np.stack([p[0] for p in pairs]).astype(dtype)
  ys = np.stack([p[1] for p in pairs]).astype(dtype)
  given = [p[2] for p in pairs]
  assert len(set(given)) > 1
  variants = [given, np.array([0.9, 250., 1.7])]
  if dtype == np.float32:
    variants.append(None)
  for ranges in variants:
    means, maps = _run(device, xs, ys, ranges)
    for i in range(3):
      one_mean, one_map = _run(device, xs[i], ys[i],
                               None if ranges is None else ranges[i])
      assert means[i] == one_mean, (i, ranges)
      assert np.array_equal(maps[i], one_map), (i, ranges)
  if dtype == np.float32:   # truth, once, for the stacked call
    means, maps = _run(device, xs, ys, given)
    for i, tag in enumerate(tags):
      _assert_close(tag + ' stacked', means[i], maps[i],
                    GOLDEN[tag + '_mean'], GOLDEN[tag + '_map'])
  # a device tensor of ranges and a scalar for all
  from utils import plotting
  dev = plotting.compute_ssim_images(
      helpers.to_dev(xs, device), helpers.to_dev(ys, device),
      torch.tensor([2., 2., 2.], dtype=torch.float64, device=device))
  scalar = plotting.compute_ssim_images(
      helpers.to_dev(xs, device), helpers.to_dev(ys, device), 2.0)
  assert torch.equal(dev, scalar)


@pytest.mark.parametrize('tag', ['range255_37x131', 'centred_17x33',
                                 'outlier_11x11', 'range1_300x11'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_identical_images_give_exactly_one(device, tag, dtype):
  x, _, r = _pair(tag) if dtype == np.float32 else _f64_pair(tag)
  mean, smap = _run(device, x, x.copy(), r)
  assert mean == 1.0
  assert (smap == 1.0).all(), int((smap != 1.0).sum())


@pytest.mark.parametrize('tag', ['range1_37x131', 'centred_37x131',
                                 'outlier_17x33', 'range255_11x300'])
def test_swapping_the_arguments(device, tag):
  x, y, r = _pair(tag)
  mean, smap = _run(device, x, y, r)
  mean_s, smap_s = _run(device, y, x, r)
  assert abs(mean - mean_s) <= SWAP_BOUND
  assert float(np.abs(smap - smap_s).max()) <= SWAP_BOUND


@pytest.mark.parametrize('tag', ['centred_37x131', 'range255_300x11'])
def test_the_same_call_twice_is_bitwise_equal(device, tag):
  x, y, r = _pair(tag)
  first = _run(device, x, y, r)
  second = _run(device, x, y, r)
  assert first[0] == second[0] and np.array_equal(first[1], second[1])
  assert first[0].tobytes() == second[0].tobytes()
