"""Writes tests/golden/code_stats.npz: the expected outputs of the
code-statistics tests for the seeded inputs of tests/code_stats_data.py.

  python tools/make_code_stats_golden.py /path/to/vision_transform_codes

The histogram truths are np.histogram / np.histogram2d / np.var /
scipy.stats.kurtosis on kept.astype(float64) with explicit float64 linspace
edges, so that the numpy version (float32 edges for float32 data under numpy
2) cannot change the answer.  The rotational_average truths come from the
reference's utils/misc.py, imported from the path given; its bin assignments,
which it does not return, are read off one-hot arrays.
"""
import pathlib
import sys
import warnings

import numpy as np
import scipy
import scipy.stats

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'tests'))
import code_stats_data as data  # noqa: E402


def narrow(counts):
  for dtype in (np.uint8, np.uint16, np.uint32):
    if counts.max(initial=0) <= np.iinfo(dtype).max:
      return counts.astype(dtype)
  return counts.astype(np.int64)


def marginal(out):
  x = data.marginal_codes()
  differs, equal_range, empty = 0, set(), set()
  for name, (ignore, overlaid) in data.VARIANTS.items():
    kept = [data.kept_values(x[:, c], ignore) for c in range(data.COLS)]
    out['kept_' + name] = narrow(np.array([len(k) for k in kept]))
    lo = np.array([k.min() if len(k) else np.nan for k in kept], np.float64)
    hi = np.array([k.max() if len(k) else np.nan for k in kept], np.float64)
    out['min_' + name], out['max_' + name] = lo, hi
    out['mean_' + name] = np.array(
        [k.astype(np.float64).mean() if len(k) else np.nan for k in kept])
    out['variance_' + name] = np.array(
        [np.var(k.astype(np.float64)) if len(k) else np.nan for k in kept])
    out['variance_f32_' + name] = np.array(
        [np.var(k) if len(k) else np.nan for k in kept], np.float32)
    if overlaid:
      lo = np.full(data.COLS, np.float64(x.min()))
      hi = np.full(data.COLS, np.float64(x.max()))
    for bins in data.BINS:
      counts = np.zeros((data.COLS, bins), np.int64)
      kurt = np.full(data.COLS, np.nan)
      for c in range(data.COLS):
        if not len(kept[c]):
          empty.add(c)
          continue
        edges = data.float64_edges(lo[c], hi[c], bins)
        counts[c] = np.histogram(kept[c].astype(np.float64), edges)[0]
        density = counts[c] / counts[c].sum()
        with warnings.catch_warnings():
          warnings.simplefilter('ignore')
          kurt[c] = scipy.stats.kurtosis(density, fisher=False)
        if lo[c] == hi[c]:
          equal_range.add(c)
          assert counts[c, -1] == len(kept[c]) and counts[c].sum() == len(kept[c])
        elif name == 'zero' and not np.array_equal(
            data.floor_formula_bins(kept[c], lo[c], hi[c], bins), counts[c]):
          differs += 1
      out['counts_%s_%d' % (name, bins)] = narrow(counts)
      out['kurtosis_%s_%d' % (name, bins)] = kurt
      if bins == 7:
        with np.errstate(invalid='ignore'):
          out['density_%s_7' % name] = counts / counts.sum(1, keepdims=True)
  # the three things that keep the fixture discriminating
  assert differs >= 1, 'no column where the uncorrected floor formula differs'
  assert data.CONSTANT in equal_range and data.LAST_ONLY in equal_range
  assert data.ALL_ZERO in empty
  out['floor_formula_differs'] = np.int64(differs)
  print('floor formula differs from np.histogram in %d (column, bins) cases'
        % differs)


def joint(out):
  x = data.marginal_codes()
  ignore = [0.0]
  kept, lo, hi = [], [], []
  for i, j in data.PAIRS:
    keep = np.ones(data.ROWS, dtype=bool)
    for v in ignore:
      keep &= (x[:, i] != np.float32(v)) & (x[:, j] != np.float32(v))
    a, b = x[keep, i].astype(np.float64), x[keep, j].astype(np.float64)
    kept.append(len(a))
    lo.append([a.min(), b.min()] if len(a) else [np.nan, np.nan])
    hi.append([a.max(), b.max()] if len(a) else [np.nan, np.nan])
    for bins in data.JOINT_BINS:
      counts = np.zeros((bins, bins), np.int64)
      if len(a):
        ex = data.float64_edges(lo[-1][0], hi[-1][0], bins)
        ey = data.float64_edges(lo[-1][1], hi[-1][1], bins)
        counts = np.histogram2d(a, b, bins=[ex, ey])[0].astype(np.int64)
        assert counts.sum() == len(a)
        if bins == 16:
          out['joint_density_%d_%d' % (i, j)] = np.histogram2d(
              a, b, bins=[ex, ey], density=True)[0]
      out['joint_counts_%d_%d_%d' % (i, j, bins)] = narrow(counts)
  out['joint_kept'] = narrow(np.array(kept))
  out['joint_lo'], out['joint_hi'] = np.array(lo), np.array(hi)
  assert kept[-1] == 0 and min(kept[:-1]) > 0


def rotational(out, reference_root):
  sys.path.insert(0, str(reference_root))
  from utils import misc as reference_misc
  for name, (h, w, nbins, _) in data.ROTATIONAL.items():
    stack, coords = data.rotational_inputs(name)
    with warnings.catch_warnings():
      warnings.simplefilter('ignore')   # the mean of an empty ring
      means = np.array([reference_misc.rotational_average(
          img, nbins, coords)[0] for img in stack])
      means32 = np.array([reference_misc.rotational_average(
          img.astype(np.float32).astype(np.float64), nbins, coords)[0]
                          for img in stack])
      edges = reference_misc.rotational_average(stack[0], nbins, coords)[1]
      # the ring of every element: the one whose mean a one-hot array moves
      assign = np.full((h, w), nbins, np.int64)
      for r in range(h):
        for c in range(w):
          probe = np.zeros((h, w))
          probe[r, c] = 1.0
          hit = np.flatnonzero(np.nan_to_num(
              reference_misc.rotational_average(probe, nbins, coords)[0]))
          assert len(hit) <= 1
          if len(hit):
            assign[r, c] = hit[0]
    out['rot_means_' + name] = means
    out['rot_means_f32_' + name] = means32
    out['rot_edges_' + name] = edges
    out['rot_assign_' + name] = narrow(assign)
    out['rot_members_' + name] = narrow(np.bincount(
        assign.reshape(-1), minlength=nbins + 1)[:nbins])
  assert np.isnan(out['rot_means_empty']).any()
  assert not np.isnan(out['rot_means_16x16']).any()


def main():
  out = {'numpy_version': np.array(np.__version__),
         'scipy_version': np.array(scipy.__version__)}
  marginal(out)
  joint(out)
  rotational(out, pathlib.Path(sys.argv[1]).resolve())
  path = REPO / 'tests' / 'golden' / 'code_stats.npz'
  np.savez_compressed(path, **out)
  largest = max(p.stat().st_size for p in path.parent.iterdir() if p != path)
  print('%s: %d bytes (largest other fixture %d)'
        % (path.name, path.stat().st_size, largest))
  assert path.stat().st_size <= min(largest, 1 << 20)


if __name__ == '__main__':
  main()
