"""
The numeric part of the reference's utils/plotting.py: compute_pSNR
(plotting.py:17-39) on device tensors.  The drawing functions and
compute_ssim of the reference are not provided.
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
