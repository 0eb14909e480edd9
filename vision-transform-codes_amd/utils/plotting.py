"""
The numeric part of the reference's utils/plotting.py on device tensors:
compute_pSNR (plotting.py:17-39) and compute_ssim (plotting.py:42-64), the
latter also for whole stacks (compute_ssim_images, csrc/ssim.hip behind
include/vtc_quality.h), and the numbers its code plots draw:
code_marginal_densities (display_code_marginal_densities, plotting.py:643-798)
and code_joint_densities (display_2d_code_densities, plotting.py:801-893),
csrc/code_stats.hip behind include/vtc_stats.h; DESIGN.md 4.14.  The drawing
functions of the reference are not provided.
"""
import numpy as np
import torch

import vtc_hip

_ROW = 4096   # elements per row handed to vtc_row_stats


def compute_pSNR(target, reconstruction, manual_sig_mag=None):
  """
  target, reconstruction : float32 tensors of one shape on a HIP device.
  manual_sig_mag : the signal range to measure the error against; when None,
      max(target) - min(target) as in the reference.
  Returns 10 log10(range^2 / MSE) as a Python float, np.inf when the two are
  equal.  The difference is formed in float32 like the reference's; its
  squares are summed in float32 over rows of 4096 elements
  (vtc_column_apply, vtc_row_stats) and the row sums in float64 on the host.
  """
  lib = vtc_hip.load_library()
  t = vtc_hip.require_device_tensor(target, 'target').contiguous()
  r = vtc_hip.require_device_tensor(reconstruction,
                                    'reconstruction').contiguous()
  assert t.shape == r.shape and t.numel() > 0
  device = t.device
  stream = vtc_hip.current_stream(device)
  total = t.numel()
  diff = torch.empty(total, dtype=torch.float32, device=device)
  vtc_hip.check(lib.vtc_column_apply(
      vtc_hip.ptr(t), vtc_hip.DTYPE_F32, 1, total, vtc_hip.COLUMN_SUBTRACT,
      vtc_hip.ptr(r), vtc_hip.ptr(diff), stream), 'vtc_column_apply')
  rows, tail = divmod(total, _ROW)
  sums = torch.empty(rows + (1 if tail else 0), dtype=torch.float32,
                     device=device)
  if rows:
    vtc_hip.check(lib.vtc_row_stats(
        vtc_hip.ptr(diff), rows, _ROW, vtc_hip.ptr(sums), vtc_hip.ptr(None),
        vtc_hip.ptr(None), stream), 'vtc_row_stats')
  if tail:
    vtc_hip.check(lib.vtc_row_stats(
        vtc_hip.ptr(diff[rows * _ROW:]), 1, tail, vtc_hip.ptr(sums[rows:]),
        vtc_hip.ptr(None), vtc_hip.ptr(None), stream), 'vtc_row_stats')
  if manual_sig_mag is None:
    minmax = torch.empty(2, dtype=torch.float32, device=device)
    ws = vtc_hip.workspace(lib.vtc_window_minmax_workspace_bytes(), device)
    vtc_hip.check(lib.vtc_window_minmax(
        vtc_hip.ptr(t), 1, 1, total, 0, 0, vtc_hip.ptr(minmax),
        vtc_hip.ptr(ws), ws.numel(), stream), 'vtc_window_minmax')
    lo, hi = minmax.cpu().numpy()
    signal_magnitude = float(hi - lo)
  else:
    signal_magnitude = float(manual_sig_mag)
  mse = float(sums.cpu().numpy().astype(np.float64).sum()) / total
  if mse != 0:
    return float(10. * np.log10(signal_magnitude**2 / mse))
  return np.inf


SSIM_WINDOW = 11   # taps per axis of the Gaussian window, sigma 1.5


def _ssim_stack(images, name):
  """A (count, h, w) float32 or float64 device tensor, contiguous, with its
  dtype code.  Shape errors come before the device check."""
  if not torch.is_tensor(images):
    raise TypeError('%s must be a torch.Tensor' % name)
  if images.dim() != 3 or images.shape[0] < 1:
    raise ValueError('%s must be (count, h, w), got shape %s'
                     % (name, tuple(images.shape)))
  if min(images.shape[1:]) < SSIM_WINDOW:
    raise ValueError('win_size exceeds image extent: %s is %d x %d, the '
                     'window has %d taps per axis'
                     % (name, images.shape[1], images.shape[2], SSIM_WINDOW))
  if images.dtype == torch.float64:
    return (vtc_hip.require_device_tensor(images, name, torch.float64)
            .contiguous(), vtc_hip.DTYPE_F64)
  return (vtc_hip.require_device_tensor(images, name).contiguous(),
          vtc_hip.DTYPE_F32)


def _own_ranges(targets):
  """(count,) float64 device tensor: max - min of each float32 target, the
  difference formed in float32 as the reference's is, then widened.  Only
  enqueues."""
  if targets.dtype != torch.float32:
    raise TypeError('manual_sig_mag=None needs float32 targets '
                    '(vtc_window_minmax reads float32); give the range of '
                    'float64 targets')
  lib = vtc_hip.load_library()
  device = targets.device
  count, h, w = targets.shape
  minmax = torch.empty((count, 2), dtype=torch.float32, device=device)
  ws = vtc_hip.workspace(lib.vtc_window_minmax_workspace_bytes(), device)
  for i in range(count):
    vtc_hip.check(lib.vtc_window_minmax(
        vtc_hip.ptr(targets[i]), 1, 1, h * w, 0, 0, vtc_hip.ptr(minmax[i]),
        vtc_hip.ptr(ws), ws.numel(), vtc_hip.current_stream(device)),
                  'vtc_window_minmax')
  return (minmax[:, 1] - minmax[:, 0]).to(torch.float64)


def _given_ranges(manual_sig_mag, count, device):
  if torch.is_tensor(manual_sig_mag):
    ranges = manual_sig_mag.to(device=device, dtype=torch.float64).reshape(-1)
  else:
    ranges = torch.from_numpy(np.ascontiguousarray(
        np.asarray(manual_sig_mag, dtype=np.float64).reshape(-1))).to(device)
  if ranges.numel() == 1:
    ranges = ranges.expand(count)
  if ranges.numel() != count:
    raise ValueError('%d ranges for %d images' % (ranges.numel(), count))
  return ranges.contiguous()


def compute_ssim_images(targets, reconstructions, manual_sig_mag=None,
                        return_map=False):
  """
  compute_ssim for every image pair of two (count, h, w) stacks, float32 or
  float64 (both stacks alike) on a HIP device.

  manual_sig_mag : the range of every image: a number, `count` of them (a
      sequence, an array or a tensor), or None for each target's own
      max - min (float32 targets).
  Returns the (count,) float64 device tensor of mean SSIMs, and with
  return_map the (count, h, w) float64 maps before cropping as well
  (scikit-image's full=True).  Only enqueues: there is no host
  synchronisation.  ValueError when a side is below 11, as in the reference.
  """
  lib = vtc_hip.load_library()
  t, code = _ssim_stack(targets, 'targets')
  r, code_r = _ssim_stack(reconstructions, 'reconstructions')
  if t.shape != r.shape:
    raise ValueError('targets %s and reconstructions %s differ in shape'
                     % (tuple(t.shape), tuple(r.shape)))
  if code != code_r:
    raise TypeError('targets are %s, reconstructions %s'
                    % (t.dtype, r.dtype))
  device = t.device
  count, h, w = t.shape
  ranges = (_own_ranges(t) if manual_sig_mag is None
            else _given_ranges(manual_sig_mag, count, device))
  means = torch.empty(count, dtype=torch.float64, device=device)
  maps = (torch.empty((count, h, w), dtype=torch.float64, device=device)
          if return_map else None)
  ws = vtc_hip.workspace(lib.vtc_ssim_workspace_bytes(count, h, w), device)
  status = lib.vtc_ssim(
      vtc_hip.ptr(t), vtc_hip.ptr(r), code, vtc_hip.ptr(ranges),
      vtc_hip.ptr(means), vtc_hip.ptr(maps), count, h, w, vtc_hip.ptr(ws),
      ws.numel(), vtc_hip.current_stream(device))
  if status == vtc_hip.ERR_UNSUPPORTED:   # the reference's ValueError
    raise ValueError('vtc_ssim: %s'
                     % lib.vtc_last_error().decode('utf-8', 'replace'))
  vtc_hip.check(status, 'vtc_ssim')
  return (means, maps) if return_map else means


def compute_ssim(target, reconstruction, manual_sig_mag=None):
  """
  target, reconstruction : 2-d float32 or float64 tensors of one shape on a
      HIP device.
  manual_sig_mag : the signal range R; when None, max(target) - min(target)
      as in the reference (the float32 difference of a float32 target).
  Returns the mean structural similarity as a Python float: scikit-image's
  compare_ssim(target, reconstruction, data_range=R, gaussian_weights=True,
  sigma=1.5, use_sample_covariance=False), computed in float64 (DESIGN.md
  4.13).  ValueError when a side is below 11.  One host read.
  """
  for name, image in (('target', target), ('reconstruction', reconstruction)):
    if not torch.is_tensor(image):
      raise TypeError('%s must be a torch.Tensor' % name)
    if image.dim() != 2:
      raise ValueError('%s must be 2-d, got shape %s'
                       % (name, tuple(image.shape)))
  return float(compute_ssim_images(target[None], reconstruction[None],
                                   manual_sig_mag)[0])


# ---------------------------------------------------------------------------
# code statistics (include/vtc_stats.h)
# ---------------------------------------------------------------------------
def _codes_2d(codes, name='codes'):
  if not torch.is_tensor(codes):
    raise TypeError('%s must be a torch.Tensor' % name)
  if codes.dim() != 2 or codes.shape[0] < 1 or codes.shape[1] < 1:
    raise ValueError('%s must be (b, s) with b, s >= 1, got shape %s'
                     % (name, tuple(codes.shape)))
  return vtc_hip.require_device_tensor(codes, name).contiguous()


def _num_bins(num_hist_bins, most):
  bins = int(num_hist_bins)
  if bins != num_hist_bins or not 1 <= bins <= most:
    raise ValueError('num_hist_bins must be an integer in 1 .. %d, got %r'
                     % (most, num_hist_bins))
  return bins


def _ignore_values(ignore_vals):
  """ignore_vals as a float32 array, the type of the codes they are compared
  with."""
  values = np.asarray(list(ignore_vals), dtype=np.float32).reshape(-1)
  if len(values) > vtc_hip.STATS_MAX_IGNORE:
    raise ValueError('at most %d ignore_vals, got %d'
                     % (vtc_hip.STATS_MAX_IGNORE, len(values)))
  return values


def _ignore_list(ignore_vals, device):
  """(device float32 tensor or None, its length)."""
  values = _ignore_values(ignore_vals)
  if not len(values):
    return None, 0
  return torch.from_numpy(values).to(device), len(values)


def _linspace_edges(lo, hi, bins):
  """np.linspace(lo, hi, bins + 1) of every row, in float64: lo + i * step,
  the product and the sum rounded separately, the last edge hi itself."""
  # a tensor divisor: dividing by a Python number multiplies by its
  # reciprocal on the device, which is not the correctly rounded quotient
  step = (hi - lo) / torch.full_like(lo, bins)
  ramp = torch.arange(bins + 1, dtype=torch.float64, device=lo.device)
  edges = ramp * step[..., None]
  edges = edges + lo[..., None]
  edges[..., -1] = hi
  return edges


def pearson_kurtosis(values):
  """scipy.stats.kurtosis(values, fisher=False) along the last axis: m4 / m2^2
  with the biased central moments, in float64."""
  centred = values - values.mean(dim=-1, keepdim=True)
  squares = centred * centred
  m2 = squares.mean(dim=-1)
  m4 = (squares * squares).mean(dim=-1)
  return m4 / (m2 * m2)


def marginal_density(counts):
  """counts / counts.sum() of every row, float64; NaN where the row is
  empty."""
  counts = counts.to(torch.float64)
  return counts / counts.sum(dim=-1, keepdim=True)


def joint_density(counts, kept, x_edges, y_edges):
  """np.histogram2d(..., density=True) from its counts: counts / kept /
  outer(diff(x_edges), diff(y_edges)) of every pair, float64."""
  area = (x_edges.diff(dim=-1)[..., :, None] *
          y_edges.diff(dim=-1)[..., None, :])
  return (counts.to(torch.float64) /
          kept.to(torch.float64)[..., None, None] / area)


def code_summary(codes, ignore_vals=[]):
  """
  Per-column statistics of (b, s) float32 device codes over the values that
  differ from every one of ignore_vals (plain !=: ignoring 0.0 drops -0.0, a
  NaN drops nothing): a dict of (s,) device tensors 'kept', 'nonfinite'
  (int64), 'min', 'max', 'mean', 'variance' (float64, ddof = 0; NaN for a
  column with nothing kept).  Only enqueues.
  """
  lib = vtc_hip.load_library()
  c = _codes_2d(codes)
  device = c.device
  b, s = c.shape
  ignore, n_ignore = _ignore_list(ignore_vals, device)
  kept, nonfinite = (torch.empty(s, dtype=torch.int64, device=device)
                     for _ in range(2))
  lo, hi, mean, var = (torch.empty(s, dtype=torch.float64, device=device)
                       for _ in range(4))
  ws = vtc_hip.workspace(lib.vtc_code_summary_workspace_bytes(b, s), device)
  vtc_hip.check(lib.vtc_code_summary(
      vtc_hip.ptr(c), b, s, vtc_hip.ptr(ignore), n_ignore, vtc_hip.ptr(kept),
      vtc_hip.ptr(lo), vtc_hip.ptr(hi), vtc_hip.ptr(mean), vtc_hip.ptr(var),
      vtc_hip.ptr(nonfinite), vtc_hip.ptr(ws), ws.numel(),
      vtc_hip.current_stream(device)), 'vtc_code_summary')
  return {'kept': kept, 'nonfinite': nonfinite, 'min': lo, 'max': hi,
          'mean': mean, 'variance': var}


def _raise_on_nonfinite(nonfinite):
  bad = np.flatnonzero(nonfinite.cpu().numpy())   # the one host read
  if len(bad):
    raise ValueError(
        'codes hold NaN or infinite values, which have no histogram range: '
        '%d columns, the first %s'
        % (len(bad), ', '.join(str(int(i)) for i in bad[:8])))


def code_marginal_densities(codes, num_hist_bins, ignore_vals=[],
                            overlaid=False):
  """
  The numbers display_code_marginal_densities draws, for every column of
  (b, s) float32 device codes at once.

  num_hist_bins : 1 .. 4096.
  ignore_vals : up to 8 values left out of every estimate (the reference's
      [0.0] for sparse codes).
  overlaid : the reference's other branch: one range for all columns, the
      minimum and maximum of the UNFILTERED matrix; the filter still applies
      to the counts.
  Returns a dict of device tensors: 'counts' (s, bins) int64, 'bin_edges'
  (s, bins + 1), 'bin_centers', 'density' (counts / counts.sum()) float64,
  'kept' int64, 'min', 'max', 'mean', 'variance' (of the kept values) and
  'kurtosis' (the reference's K: the Pearson kurtosis of the density vector)
  float64.  The counts are np.histogram(kept.astype(float64),
  np.linspace(lo, hi, bins + 1)) exactly.

  Where the reference would raise from min([]), a column with nothing kept
  gives zero counts and NaN edges, density, variance and kurtosis: with 1024
  atoms a dead one is ordinary.  NaN or infinite codes raise ValueError, as
  np.histogram does for such a range; finding out is the one host read.
  """
  lib = vtc_hip.load_library()
  bins = _num_bins(num_hist_bins, vtc_hip.STATS_MAX_BINS)
  _ignore_values(ignore_vals)
  c = _codes_2d(codes)
  device = c.device
  b, s = c.shape
  ignore, n_ignore = _ignore_list(ignore_vals, device)
  summary = code_summary(c, ignore_vals)
  lo, hi = summary['min'], summary['max']
  nonfinite = summary['nonfinite']
  if overlaid:
    whole = code_summary(c) if n_ignore else summary
    nonfinite = nonfinite + whole['nonfinite']
  _raise_on_nonfinite(nonfinite)
  if overlaid:
    lo = whole['min'].min().expand(s).contiguous()
    hi = whole['max'].max().expand(s).contiguous()
  counts = torch.empty((s, bins), dtype=torch.int64, device=device)
  ws = vtc_hip.workspace(lib.vtc_code_histogram_workspace_bytes(b, s, bins),
                         device)
  vtc_hip.check(lib.vtc_code_histogram(
      vtc_hip.ptr(c), b, s, vtc_hip.ptr(ignore), n_ignore, vtc_hip.ptr(lo),
      vtc_hip.ptr(hi), bins, vtc_hip.ptr(counts), vtc_hip.ptr(ws), ws.numel(),
      vtc_hip.current_stream(device)), 'vtc_code_histogram')
  edges = _linspace_edges(lo, hi, bins)
  density = marginal_density(counts)
  return {'counts': counts, 'bin_edges': edges,
          'bin_centers': (edges[:, :-1] + edges[:, 1:]) / 2,
          'density': density, 'kept': summary['kept'], 'min': summary['min'],
          'max': summary['max'], 'mean': summary['mean'],
          'variance': summary['variance'],
          'kurtosis': pearson_kurtosis(density)}


def code_joint_densities(codes, pairs, num_hist_bins, ignore_vals=[]):
  """
  The joint density display_2d_code_densities draws, for a list of column
  pairs of (b, s) float32 device codes in one call.

  pairs : sequence of (i, j) column indices; one outside [0, s) raises
      ValueError.
  num_hist_bins : 1 .. 256 per axis.
  ignore_vals : a row is left out of a pair when either of its two values
      equals one of these.
  Returns a dict of device tensors: 'counts' (P, bins, bins) int64, the first
  axis the first column of the pair; 'x_edges', 'y_edges' (P, bins + 1)
  float64, np.linspace over the kept rows' range of each axis; 'density'
  (P, bins, bins) float64 = np.histogram2d(..., density=True); 'kept' (P,)
  int64.  A pair with no row kept gives zero counts and NaN edges and
  density.  Only enqueues.
  """
  lib = vtc_hip.load_library()
  bins = _num_bins(num_hist_bins, vtc_hip.STATS_MAX_JOINT_BINS)
  _ignore_values(ignore_vals)
  c = _codes_2d(codes)
  device = c.device
  b, s = c.shape
  table = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
  if len(table) < 1:
    raise ValueError('pairs is empty')
  if table.min() < 0 or table.max() >= s:
    raise ValueError('pairs name a column outside 0 .. %d' % (s - 1))
  p = len(table)
  ignore, n_ignore = _ignore_list(ignore_vals, device)
  table = torch.from_numpy(table.astype(np.int32)).to(device)
  kept = torch.empty(p, dtype=torch.int64, device=device)
  lo, hi = (torch.empty((p, 2), dtype=torch.float64, device=device)
            for _ in range(2))
  counts = torch.empty((p, bins, bins), dtype=torch.int64, device=device)
  ws = vtc_hip.workspace(
      lib.vtc_code_joint_histogram_workspace_bytes(b, p), device)
  vtc_hip.check(lib.vtc_code_joint_histogram(
      vtc_hip.ptr(c), b, s, vtc_hip.ptr(table), p, s, vtc_hip.ptr(ignore),
      n_ignore, bins, vtc_hip.ptr(kept), vtc_hip.ptr(lo), vtc_hip.ptr(hi),
      vtc_hip.ptr(counts), vtc_hip.ptr(ws), ws.numel(),
      vtc_hip.current_stream(device)), 'vtc_code_joint_histogram')
  x_edges = _linspace_edges(lo[:, 0], hi[:, 0], bins)
  y_edges = _linspace_edges(lo[:, 1], hi[:, 1], bins)
  return {'counts': counts, 'x_edges': x_edges, 'y_edges': y_edges,
          'density': joint_density(counts, kept, x_edges, y_edges),
          'kept': kept}


def code_joint_density(two_codes, num_hist_bins, ignore_vals=[]):
  """code_joint_densities for the reference's (D, 2) argument: the same dict
  without the leading pair axis."""
  c = _codes_2d(two_codes, 'two_codes')
  if c.shape[1] != 2:
    raise ValueError('two_codes must be (D, 2), got shape %s'
                     % (tuple(c.shape),))
  out = code_joint_densities(c, [(0, 1)], num_hist_bins, ignore_vals)
  return {k: v[0] for k, v in out.items()}
