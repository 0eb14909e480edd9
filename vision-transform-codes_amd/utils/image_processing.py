"""
Image whitening on MI355X: the step before the sparse-coding path.

Device counterpart of whiten_center_surround in vision_transform_codes/utils/
image_processing.py:267-308 (filter_fd :63-92, get_low_pass_filter :173-231,
get_whitening_ramp_filter :234-264): rolled-off ramp times an order-8
exponential low-pass, applied in the frequency domain in float64 (hipFFT) and
returned as float32, as the reference does with numpy.

ZCA whitening (whiten_ZCA / unwhiten_ZCA, the reference's :338-460): float64
covariance, Jacobi eigen-decomposition and the ZCA matrix on the device
(vtc_hip.linalg, csrc/zca.hip), then one float32 row transform of the data.
"""
import numpy as np
import torch

import vtc_hip
from vtc_hip import linalg

ZCA_EPS = 1e-4   # image_processing.py:412, :454


def whiten_center_surround(image, cutoffs, return_filter=False,
                           norm_and_threshold=True):
  """
  image : float32 tensor on a HIP device, (h, w, c) like the reference, or a
      stack (count, h, w, c) of equally sized images (an extension: one
      batched transform).
  cutoffs : {'low': ..., 'high': ...} as in the reference.
  norm_and_threshold : as in the reference (default True: the transfer
      function is divided by its maximum and floored at 1e-3; the dataset
      pipeline, dataset_generation.py:231-238, passes False).
  Returns the filtered image(s), same shape.  return_filter=True is host-side
  debugging output and not implemented on the device.
  """
  if return_filter:
    raise NotImplementedError('return_filter is host-side debugging output')
  lib = vtc_hip.load_library()
  image = vtc_hip.require_device_tensor(image, 'image').contiguous()
  assert image.dim() in (3, 4), 'expected (h, w, c) or (count, h, w, c)'
  stacked = image if image.dim() == 4 else image[None]
  count, h, w, c = stacked.shape
  out = torch.empty_like(stacked)
  ws = vtc_hip.workspace(
      lib.vtc_whiten_center_surround_workspace_bytes(count, h, w, c),
      image.device)
  vtc_hip.check(lib.vtc_whiten_center_surround(
      vtc_hip.ptr(stacked), vtc_hip.ptr(out), count, h, w, c,
      float(cutoffs['low']), float(cutoffs['high']),
      1 if norm_and_threshold else 0, vtc_hip.ptr(ws), ws.numel(),
      vtc_hip.current_stream(image.device)), 'vtc_whiten_center_surround')
  return out if image.dim() == 4 else out[0]


def _zca_input(flat_data, name):
  """A (D, n) device tensor as float32: float32 as is, uint8 by an exact cast
  (the reference accepts both, image_processing.py:380)."""
  if torch.is_tensor(flat_data) and flat_data.dtype == torch.uint8:
    flat_data = vtc_hip.require_device_tensor(flat_data, name, torch.uint8)
    flat_data = flat_data.to(torch.float32)
  x = vtc_hip.require_device_tensor(flat_data, name).contiguous()
  assert x.dim() == 2, '%s must be (D, n)' % name
  return x


def _device_parameters(params, n, device):
  """(U float32 (n, n), w float64 (n,), m as a float32-valued Python float)
  from a ZCA parameter dict holding device tensors or the reference's numpy
  arrays."""
  def dev(v, dtype):
    if not torch.is_tensor(v):
      v = torch.from_numpy(np.ascontiguousarray(np.asarray(v)))
    return v.to(device=device).to(dtype).contiguous()
  u = dev(params['PCA_basis'], torch.float32)
  w = dev(params['PCA_axis_variances'], torch.float64)
  m = params['subtracted_mean']
  m = float(m.item()) if torch.is_tensor(m) else float(np.float32(m))
  assert u.shape == (n, n) and w.shape == (n,), 'parameters do not match n'
  return u, w, m


def whiten_ZCA(flat_data, precomputed_ZCA_parameters=None):
  """
  The reference's whiten_ZCA (image_processing.py:338-416) on the device.

  flat_data : (D, n) float32 or uint8 tensor on a HIP device.
  precomputed_ZCA_parameters : None (estimate them from flat_data), or a dict
      with the reference's keys 'PCA_basis' (n, n), 'PCA_axis_variances' (n,)
      and 'subtracted_mean' (scalar), as device tensors or numpy arrays (so
      parameters estimated by the reference can be used).

  Returns the whitened (D, n) float32 device tensor and, when estimating, the
  parameter dict (device tensors: 'PCA_basis' (n, n) float32 with the
  principal directions as columns, 'PCA_axis_variances' (n,) float32 in
  descending order, 'subtracted_mean' a 0-d float32 tensor).

  Semantics kept from the reference, including its asymmetry: the estimating
  call whitens data centred per component, y = (x - mu) W + m, and stores
  m = mean(mu); a call with parameters and unwhiten_ZCA subtract the scalar m
  instead.  W = U diag(1/(sqrt(w) + 1e-4)) U^T is formed in float64 and
  rounded to float32 (the reference's two products with U, as one matrix).
  The covariance is float64 (the reference: float32); the eigenvectors follow
  the sign rule of vtc_sym_eig (the reference's are LAPACK's, arbitrary), W
  does not depend on it.  n > 256, or a Jacobi run that does not converge,
  takes torch.linalg.eigh (vtc_hip.linalg.symmetric_eigh).
  """
  x = _zca_input(flat_data, 'flat_data')
  num_samples, num_components = x.shape
  if precomputed_ZCA_parameters is None:
    if num_components > 0.1 * num_samples:
      raise RuntimeError('Number of samples is way too small to estimate PCA')
    cov, means, grand = linalg.column_covariance(x, center=True)
    w, u = linalg.symmetric_eigh(cov)
    w_mat, _ = linalg.zca_matrices(u, w, ZCA_EPS, unwhiten=False)
    subtracted_mean = grand.to(torch.float32).reshape(())
    params = {'PCA_basis': u, 'PCA_axis_variances': w.to(torch.float32),
              'subtracted_mean': subtracted_mean}
    white = linalg.row_transform(x, means.to(torch.float32), w_mat,
                                 float(subtracted_mean.item()))
    return white, params
  u, w, m = _device_parameters(precomputed_ZCA_parameters, num_components,
                               x.device)
  w_mat, _ = linalg.zca_matrices(u, w, ZCA_EPS, unwhiten=False)
  offsets = torch.full((num_components,), m, dtype=torch.float32,
                       device=x.device)
  return linalg.row_transform(x, offsets, w_mat, m)


def unwhiten_ZCA(white_flat_data, precomputed_ZCA_parameters):
  """
  The reference's unwhiten_ZCA (image_processing.py:419-460) on the device:
  y = (x - m) W^-1 + m with W^-1 = U diag(sqrt(w) + 1e-4) U^T (float64,
  rounded to float32) and m the parameters' 'subtracted_mean'.  Parameters
  as for whiten_ZCA (device tensors or the reference's numpy arrays).  As in
  the reference, this does not invert an ESTIMATING whiten_ZCA call exactly:
  that call centred each component by its own mean.
  """
  x = vtc_hip.require_device_tensor(white_flat_data,
                                    'white_flat_data').contiguous()
  num_components = x.shape[1]
  u, w, m = _device_parameters(precomputed_ZCA_parameters, num_components,
                               x.device)
  _, w_inv = linalg.zca_matrices(u, w, ZCA_EPS, whiten=False)
  offsets = torch.full((num_components,), m, dtype=torch.float32,
                       device=x.device)
  return linalg.row_transform(x, offsets, w_inv, m)
