"""
The numeric part of the reference's utils/plotting.py on device tensors:
compute_pSNR (plotting.py:17-39) and compute_ssim (plotting.py:42-64), the
latter also for whole stacks (compute_ssim_images, csrc/ssim.hip behind
include/vtc_quality.h).  The drawing functions of the
reference are not provided.
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
