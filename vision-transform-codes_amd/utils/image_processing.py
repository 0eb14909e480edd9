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

Local contrast normalisation / local luminance subtraction (the reference's
:463-523 with filter_sd :18-60 and get_gaussian_filter_2d :136-170) and the
component / sample statistics (:526-590): csrc/local_norm.hip.
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


def gaussian_window(filter_sigma):
  """(first coordinate, tap count) of the reference's
  get_gaussian_filter_2d(filter_sigma, (4 sigma + 1, 4 sigma + 1)) along one
  axis.  Host only; raises ValueError for a sigma that is not a positive
  number or whose window has an even number of taps (an off-centre window,
  which the separable device filter does not take)."""
  if (isinstance(filter_sigma, (bool, np.bool_)) or
      not isinstance(filter_sigma, (int, float, np.integer, np.floating)) or
      not 0 < filter_sigma < 1e7):
    raise ValueError('filter_sigma must be a positive number below 1e7, got '
                     '%r' % (filter_sigma,))
  window = 4 * filter_sigma + 1
  lower = -int(np.floor(window / 2))
  upper = int(np.floor(window / 2)) + (1 if window % 2 != 0 else 0)
  taps = upper - lower
  if taps % 2 == 0:
    raise ValueError('filter_sigma %r gives a window of %d taps: only odd '
                     'windows (centred on the pixel) are supported'
                     % (filter_sigma, taps))
  return lower, taps


def _local_normalize(image, filter_sigma, mode):
  gaussian_window(filter_sigma)
  lib = vtc_hip.load_library()
  image = vtc_hip.require_device_tensor(image, 'image').contiguous()
  assert image.dim() in (3, 4), 'expected (h, w, c) or (count, h, w, c)'
  stacked = image if image.dim() == 4 else image[None]
  count, h, w, c = stacked.shape
  out = torch.empty_like(stacked)
  aux = torch.empty_like(stacked)
  if stacked.numel():
    ws = vtc_hip.workspace(lib.vtc_local_normalize_workspace_bytes(
        count, h, w, c, float(filter_sigma)), image.device)
    vtc_hip.check(lib.vtc_local_normalize(
        vtc_hip.ptr(stacked), vtc_hip.ptr(out), vtc_hip.ptr(aux), count, h, w,
        c, float(filter_sigma), mode, vtc_hip.ptr(ws), ws.numel(),
        vtc_hip.current_stream(image.device)), 'vtc_local_normalize')
  if image.dim() == 3:
    out, aux = out[0], aux[0]
  return out, aux


def local_contrast_normalization(image, filter_sigma, return_normalizer=False):
  """
  The reference's local_contrast_normalization (image_processing.py:463-493)
  on the device.

  image : float32 tensor on a HIP device, (h, w, c) or a stack
      (count, h, w, c) of equally sized images (an extension).
  filter_sigma : the Gaussian's standard deviation; the window is
      4 sigma + 1 taps wide and must have an odd tap count.
  Returns image / sqrt(v) and, with return_normalizer, sqrt(v), where v is
  the float32 square of the image filtered with the reference's window
  (float64 sums, scipy's 'symm' boundary), 0 replaced by 1.
  """
  out, aux = _local_normalize(image, filter_sigma, vtc_hip.LOCAL_CONTRAST)
  return (out, aux) if return_normalizer else out


def local_luminance_subtraction(image, filter_sigma, return_subtractor=False):
  """
  The reference's local_luminance_subtraction (image_processing.py:496-523)
  on the device: image - g * image with the same window and boundary as
  local_contrast_normalization; return_subtractor adds g * image (float32).
  """
  out, aux = _local_normalize(image, filter_sigma, vtc_hip.LOCAL_LUMINANCE)
  return (out, aux) if return_subtractor else out


def _stat_input(flat_data, name):
  """A (D, n) float32 or uint8 device tensor and its vtc_dtype code (the
  reference accepts both, image_processing.py:544, :567, :590)."""
  if torch.is_tensor(flat_data) and flat_data.dtype == torch.uint8:
    x = vtc_hip.require_device_tensor(flat_data, name, torch.uint8)
    code = vtc_hip.DTYPE_U8
  else:
    x = vtc_hip.require_device_tensor(flat_data, name)
    code = vtc_hip.DTYPE_F32
  assert x.dim() == 2 and x.shape[0] > 0 and x.shape[1] > 0, (
      '%s must be a non-empty (D, n)' % name)
  return x.contiguous(), code


def _column_moments(x, code, want_var):
  lib = vtc_hip.load_library()
  rows, cols = x.shape
  mean = torch.empty(cols, dtype=torch.float32, device=x.device)
  var = torch.empty_like(mean) if want_var else None
  ws = vtc_hip.workspace(lib.vtc_column_moments_workspace_bytes(rows, cols),
                         x.device)
  vtc_hip.check(lib.vtc_column_moments(
      vtc_hip.ptr(x), code, rows, cols, vtc_hip.ptr(mean), vtc_hip.ptr(var),
      vtc_hip.ptr(ws), ws.numel(), vtc_hip.current_stream(x.device)),
      'vtc_column_moments')
  return mean, var


def _column_apply(x, code, op, v):
  out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
  vtc_hip.check(vtc_hip.load_library().vtc_column_apply(
      vtc_hip.ptr(x), code, x.shape[0], x.shape[1], op, vtc_hip.ptr(v),
      vtc_hip.ptr(out), vtc_hip.current_stream(x.device)), 'vtc_column_apply')
  return out


def center_each_component(flat_data):
  """The reference's center_each_component (image_processing.py:527-547):
  flat_data (D, n) float32 or uint8 on the device -> (flat_data - means as
  float32, means (n,) float32).  Means are float64 sums rounded to float32."""
  x, code = _stat_input(flat_data, 'flat_data')
  mean, _ = _column_moments(x, code, want_var=False)
  return _column_apply(x, code, vtc_hip.COLUMN_SUBTRACT, mean), mean


def normalize_component_variance(flat_data):
  """The reference's normalize_component_variance (image_processing.py:
  573-594): (flat_data / sqrt(variances), variances (n,) float32), ddof = 0;
  a zero-variance column is not guarded, as in the reference."""
  x, code = _stat_input(flat_data, 'flat_data')
  _, var = _column_moments(x, code, want_var=True)
  return _column_apply(x, code, vtc_hip.COLUMN_DIVIDE_SQRT, var), var


def center_each_sample(flat_data):
  """The reference's center_each_sample (image_processing.py:550-570):
  (flat_data - row means, row means (D,) float32)."""
  x, code = _stat_input(flat_data, 'flat_data')
  out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
  means = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
  vtc_hip.check(vtc_hip.load_library().vtc_row_center(
      vtc_hip.ptr(x), code, x.shape[0], x.shape[1], vtc_hip.ptr(out),
      vtc_hip.ptr(means), vtc_hip.current_stream(x.device)), 'vtc_row_center')
  return out, means
