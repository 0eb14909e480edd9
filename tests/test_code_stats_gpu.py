"""Code statistics on the device (include/vtc_stats.h, utils.plotting,
utils.misc) against tests/golden/code_stats.npz, whose truths are np.histogram
/ np.histogram2d / np.var / scipy.stats.kurtosis on float64 values with
explicit float64 linspace edges, and the reference's rotational_average
(tools/make_code_stats_golden.py).  The inputs are the seeded arrays of
tests/code_stats_data.py.

Counts, kept, min, max and bin edges are EQUAL to the truth.  Mean and variance
are within 1e-11 relative: a float64 sum of <= 4099 terms is off by at most
4099 * 2^-53 = 4.6e-13 of the sum of magnitudes, the rest is margin (for the
mean, relative to mean |x|).  Every call is made twice and compared bitwise.
"""
import numpy as np
import pytest
import torch

import code_stats_data as data
import helpers

pytestmark = pytest.mark.gpu

BOUND = 1e-11


def same_bits(a, b):
  """torch.equal that takes NaN for what it is: a bit pattern."""
  if a.dtype == torch.float64:
    a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
  return a.shape == b.shape and bool(torch.equal(a, b))


def twice(fn):
  first, second = fn(), fn()
  if isinstance(first, dict):
    for k in first:
      assert same_bits(first[k], second[k]), '%s differs between two calls' % k
  else:
    for n, (a, b) in enumerate(zip(first, second)):
      if torch.is_tensor(a):
        assert same_bits(a, b), 'output %d differs between two calls' % n
  return first


def host(result):
  return {k: v.cpu().numpy() for k, v in result.items()}


@pytest.fixture(scope='module')
def golden():
  return helpers.load('code_stats')


@pytest.fixture(scope='module')
def codes():
  return data.marginal_codes()


@pytest.fixture(scope='module')
def codes_dev(codes, device):
  return torch.from_numpy(codes).to(device)


def close(got, want, scale=None):
  """NaN in the same places, elsewhere |got - want| <= BOUND * scale."""
  assert np.array_equal(np.isnan(got), np.isnan(want))
  ok = ~np.isnan(want)
  scale = np.abs(want) if scale is None else scale
  gap = np.abs(got[ok] - want[ok])
  assert (gap <= BOUND * scale[ok]).all(), float(
      (gap / np.maximum(scale[ok], 1e-300)).max())


def check_marginal(result, g, x, name, bins, ignore, overlaid):
  r = host(result)
  assert r['counts'].dtype == np.int64 and r['counts'].shape == (x.shape[1],
                                                                 bins)
  assert np.array_equal(r['counts'], g['counts_%s_%d' % (name, bins)])
  assert np.array_equal(r['kept'], g['kept_' + name])
  assert np.array_equal(r['min'], g['min_' + name], equal_nan=True)
  assert np.array_equal(r['max'], g['max_' + name], equal_nan=True)
  lo, hi = g['min_' + name], g['max_' + name]
  if overlaid:
    lo = np.full(len(lo), np.float64(x.min()))
    hi = np.full(len(hi), np.float64(x.max()))
  edges = np.stack([data.float64_edges(a, b, bins) for a, b in zip(lo, hi)])
  assert np.array_equal(r['bin_edges'].view(np.int64), edges.view(np.int64))
  assert np.array_equal(r['bin_centers'], (edges[:, :-1] + edges[:, 1:]) / 2,
                        equal_nan=True)
  mean_abs = np.array([np.abs(data.kept_values(x[:, c], ignore)).astype(
      np.float64).mean() if g['kept_' + name][c] else np.nan
                       for c in range(x.shape[1])])
  close(r['mean'], g['mean_' + name], mean_abs)
  close(r['variance'], g['variance_' + name])
  close(r['kurtosis'], g['kurtosis_%s_%d' % (name, bins)])
  with np.errstate(invalid='ignore'):
    density = r['counts'] / r['counts'].sum(1, keepdims=True)
  assert np.array_equal(r['density'], density, equal_nan=True)
  ok = ~np.isnan(g['variance_' + name]) & (g['variance_' + name] > 0)
  f32_gap = np.abs(g['variance_f32_' + name][ok].astype(np.float64) -
                   g['variance_' + name][ok]) / g['variance_' + name][ok]
  print('code_stats %s bins %d: reference float32 np.var is off by %.1e '
        'relative at most (not gated)' % (name, bins, f32_gap.max()))


@pytest.mark.parametrize('bins', data.BINS)
@pytest.mark.parametrize('name', sorted(data.VARIANTS))
def test_marginal_densities(codes, codes_dev, golden, name, bins):
  from utils import plotting
  ignore, overlaid = data.VARIANTS[name]
  result = twice(lambda: plotting.code_marginal_densities(
      codes_dev, bins, ignore, overlaid))
  check_marginal(result, golden, codes, name, bins, ignore, overlaid)
  # a column with nothing kept: zero counts, NaN everywhere else
  if name != 'none':
    r = host(result)
    assert not r['counts'][data.ALL_ZERO].any()
    assert np.isnan(r['density'][data.ALL_ZERO]).all()
    assert np.isnan(r['variance'][data.ALL_ZERO])
    if not overlaid:
      assert np.isnan(r['bin_edges'][data.ALL_ZERO]).all()
      # lo == hi: everything in the last bin
      assert r['counts'][data.CONSTANT, -1] == data.ROWS
      assert r['counts'][data.LAST_ONLY].tolist() == [0] * (bins - 1) + [1]


@pytest.mark.parametrize('bins', data.BINS)
def test_a_nan_in_the_ignore_list_drops_nothing(codes, codes_dev, golden,
                                                bins):
  from utils import plotting
  result = twice(lambda: plotting.code_marginal_densities(
      codes_dev, bins, [0.0, float('nan')]))
  check_marginal(result, golden, codes, 'zero', bins, [0.0], False)


def _numpy_marginal(x, bins, ignore):
  out = {'counts': np.zeros((x.shape[1], bins), np.int64),
         'kept': np.zeros(x.shape[1], np.int64)}
  for c in range(x.shape[1]):
    kept = data.kept_values(x[:, c], ignore)
    out['kept'][c] = len(kept)
    if len(kept):
      out['counts'][c] = np.histogram(
          kept.astype(np.float64),
          data.float64_edges(kept.min(), kept.max(), bins))[0]
  return out


@pytest.mark.parametrize('b,s', ((1, 1), (1, 70), (65537, 3), (5, 4096)))
def test_edges_of_the_shape(device, b, s):
  """One row, one column, rows past 2^16 in three columns (a tile that is
  nearly all padding), and 4096 columns of five rows."""
  from utils import plotting
  rs = np.random.RandomState(b + s)
  x = rs.laplace(size=(b, s)).astype(np.float32)
  x[rs.rand(b, s) < 0.5] = 0.0
  x[0, 0] = 0.75
  xd = torch.from_numpy(x).to(device)
  for bins in (1, 100, 4096):
    result = host(twice(lambda: plotting.code_marginal_densities(
        xd, bins, [0.0])))
    want = _numpy_marginal(x, bins, [0.0])
    assert np.array_equal(result['counts'], want['counts']), bins
    assert np.array_equal(result['kept'], want['kept'])
    assert result['counts'].sum() == (x != 0).sum()


def test_nonfinite_codes(codes, codes_dev, golden, device):
  """+-inf or NaN raise ValueError naming the column; the C calls themselves
  answer VTC_OK with `nonfinite` set, leave the values out and get the other
  columns right."""
  import vtc_hip
  from utils import plotting
  bad = codes.copy()
  bad[5, 3], bad[77, 3], bad[4098, 3] = np.inf, np.nan, -np.inf
  bad_dev = torch.from_numpy(bad).to(device)
  with pytest.raises(ValueError, match=r'first 3\b'):
    plotting.code_marginal_densities(bad_dev, 7, [0.0])
  with pytest.raises(ValueError, match=r'first 3\b'):
    plotting.code_marginal_densities(bad_dev, 7, [], overlaid=True)

  summary = twice(lambda: plotting.code_summary(bad_dev, [0.0]))
  r = host(summary)
  assert r['nonfinite'].tolist() == [3 if c == 3 else 0
                                     for c in range(data.COLS)]
  fine = data.kept_values(bad[:, 3], [0.0])
  assert r['kept'][3] == len(fine)
  fine = fine[np.isfinite(fine)].astype(np.float64)
  assert r['min'][3] == fine.min() and r['max'][3] == fine.max()
  assert abs(r['mean'][3] - fine.mean()) <= BOUND * np.abs(fine).mean()
  assert abs(r['variance'][3] - fine.var()) <= BOUND * fine.var()
  others = np.arange(data.COLS) != 3
  for key, name in (('kept', 'kept_zero'), ('min', 'min_zero'),
                    ('max', 'max_zero')):
    assert np.array_equal(r[key][others], golden[name][others],
                          equal_nan=True)

  lib = vtc_hip.load_library()
  bins = 7
  ignore = torch.zeros(1, dtype=torch.float32, device=device)
  ws = vtc_hip.workspace(
      lib.vtc_code_histogram_workspace_bytes(data.ROWS, data.COLS, bins),
      device)

  def raw_histogram():
    counts = torch.full((data.COLS, bins), -1, dtype=torch.int64,
                        device=device)
    rc = lib.vtc_code_histogram(
        vtc_hip.ptr(bad_dev), data.ROWS, data.COLS, vtc_hip.ptr(ignore), 1,
        vtc_hip.ptr(summary['min']), vtc_hip.ptr(summary['max']), bins,
        vtc_hip.ptr(counts), vtc_hip.ptr(ws), ws.numel(),
        vtc_hip.current_stream(device))
    torch.cuda.synchronize(device)
    assert rc == 0, lib.vtc_last_error()
    return {'counts': counts}

  counts = twice(raw_histogram)['counts'].cpu().numpy()
  assert np.array_equal(counts[others], golden['counts_zero_7'][others])
  assert np.array_equal(counts[3], np.histogram(
      fine, data.float64_edges(fine.min(), fine.max(), bins))[0])


@pytest.mark.parametrize('bins', data.JOINT_BINS)
def test_joint_densities(codes_dev, golden, bins):
  from utils import plotting
  result = host(twice(lambda: plotting.code_joint_densities(
      codes_dev, data.PAIRS, bins, [0.0])))
  assert np.array_equal(result['kept'], golden['joint_kept'])
  for n, pair in enumerate(data.PAIRS):
    want = golden['joint_counts_%d_%d_%d' % (pair + (bins,))]
    assert np.array_equal(result['counts'][n], want), pair
    for axis, key in enumerate(('x_edges', 'y_edges')):
      edges = data.float64_edges(golden['joint_lo'][n, axis],
                                 golden['joint_hi'][n, axis], bins)
      assert np.array_equal(result[key][n].view(np.int64),
                            edges.view(np.int64)), (pair, key)
    if bins == 16 and golden['joint_kept'][n]:
      truth = golden['joint_density_%d_%d' % pair]
      assert (np.abs(result['density'][n] - truth) <= BOUND * truth).all()
  # the pair whose filtered rows are empty
  assert not result['counts'][-1].any()
  assert np.isnan(result['x_edges'][-1]).all()
  assert np.isnan(result['y_edges'][-1]).all()
  # (5, 5): the diagonal
  diagonal = result['counts'][1]
  assert diagonal.sum() == np.trace(diagonal) == golden['joint_kept'][1]


def test_joint_of_two_codes(codes, codes_dev, golden):
  from utils import plotting
  two = codes_dev[:, [10, 11]].contiguous()
  result = host(twice(lambda: plotting.code_joint_density(two, 64, [0.0])))
  assert np.array_equal(result['counts'], golden['joint_counts_10_11_64'])
  assert result['kept'] == golden['joint_kept'][3]


def test_joint_pair_outside_the_columns(codes_dev, golden, device):
  """Python refuses the list before uploading it; through the raw C call the
  pair's kept is -1, its counts zero, and the other pairs are unchanged."""
  import vtc_hip
  from utils import plotting
  for pair in ((0, 70), (70, 0), (-1, 3)):
    with pytest.raises(ValueError):
      plotting.code_joint_densities(codes_dev, [(0, 1), pair], 16, [0.0])
  lib = vtc_hip.load_library()
  bins = 16
  pairs = np.array([(0, 1), (0, 70), (69, 0), (-1, 3)], np.int32)
  p = len(pairs)
  pairs_dev = torch.from_numpy(pairs).to(device)
  ignore = torch.zeros(1, dtype=torch.float32, device=device)
  ws = vtc_hip.workspace(
      lib.vtc_code_joint_histogram_workspace_bytes(data.ROWS, p), device)

  def raw_joint():
    kept = torch.full((p,), 7, dtype=torch.int64, device=device)
    lo, hi = (torch.zeros((p, 2), dtype=torch.float64, device=device)
              for _ in range(2))
    counts = torch.full((p, bins, bins), -1, dtype=torch.int64, device=device)
    rc = lib.vtc_code_joint_histogram(
        vtc_hip.ptr(codes_dev), data.ROWS, data.COLS, vtc_hip.ptr(pairs_dev),
        p, data.COLS, vtc_hip.ptr(ignore), 1, bins, vtc_hip.ptr(kept),
        vtc_hip.ptr(lo), vtc_hip.ptr(hi), vtc_hip.ptr(counts),
        vtc_hip.ptr(ws), ws.numel(), vtc_hip.current_stream(device))
    torch.cuda.synchronize(device)
    assert rc == 0, lib.vtc_last_error()
    return {'kept': kept, 'lo': lo, 'hi': hi, 'counts': counts}

  result = twice(raw_joint)
  kept, lo, hi, counts = (result[k] for k in ('kept', 'lo', 'hi', 'counts'))
  kept, counts = kept.cpu().numpy(), counts.cpu().numpy()
  assert kept.tolist() == [int(golden['joint_kept'][0]), -1,
                           int(golden['joint_kept'][2]), -1]
  assert np.array_equal(counts[0], golden['joint_counts_0_1_16'])
  assert np.array_equal(counts[2], golden['joint_counts_69_0_16'])
  assert not counts[1].any() and not counts[3].any()
  assert np.isnan(lo.cpu().numpy()[[1, 3]]).all()
  assert np.isnan(hi.cpu().numpy()[[1, 3]]).all()
  assert np.array_equal(lo.cpu().numpy()[[0, 2]], golden['joint_lo'][[0, 2]])


@pytest.mark.parametrize('dtype', (np.float32, np.float64),
                         ids=('f32', 'f64'))
@pytest.mark.parametrize('name', sorted(data.ROTATIONAL))
def test_rotational_average(golden, device, name, dtype):
  from utils import misc
  h, w, nbins, _ = data.ROTATIONAL[name]
  stack, coords = data.rotational_inputs(name)
  want = golden['rot_means_%s%s' % ('f32_' if dtype == np.float32 else '',
                                    name)]
  on_device = torch.from_numpy(stack.astype(dtype)).to(device)
  means, edges = twice(lambda: misc.rotational_average(on_device, nbins,
                                                       coords))
  assert means.dtype == torch.float64 and tuple(means.shape) == (data.STACK,
                                                                 nbins)
  assert np.array_equal(edges, golden['rot_edges_' + name])
  close(means.cpu().numpy(), want)
  # one image: the reference's signature and return pair
  single, _ = twice(lambda: misc.rotational_average(on_device[1], nbins,
                                                    coords))
  assert same_bits(single, means[1])
  bin_of, _ = misc.rotational_bin_map((h, w), nbins, coords)
  _, members = twice(lambda: misc.binned_mean(
      on_device, torch.from_numpy(bin_of.copy()).to(device), nbins))
  assert np.array_equal(members.cpu().numpy(), golden['rot_members_' + name])
  if name == 'empty':   # NaN in the empty rings and nowhere else
    assert np.array_equal(np.isnan(means.cpu().numpy()),
                          np.broadcast_to(golden['rot_members_empty'] == 0,
                                          (data.STACK, nbins)))
    assert (golden['rot_members_empty'] == 0).any()
