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

The image-level half -- filter_fd (:63-92), filter_sd (:18-60), downsample
(:95-114), patches_from_single_image / assemble_image_from_patches (:597-699)
and unwhiten_center_surround (:311-335): csrc/image_tools.hip, declared in
include/vtc_image.h.  The filter builders (:117-264) are host-side numpy, as
in the reference.
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
  debugging output and not implemented on the device: it raises
  NotImplementedError.  center_surround_filter(image.shape, cutoffs,
  norm_and_threshold) returns the same transfer function, which is what
  unwhiten_center_surround(orig_filter_DFT=...) takes.
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


# ---------------------------------------------------------------------------
# The image-level half (include/vtc_image.h, csrc/image_tools.hip): a caller's
# own filters, downsampling, tiling an image into patches and back, and
# undoing center-surround whitening.
# ---------------------------------------------------------------------------
def _image_input(image, name):
  """A (h, w, c) or (count, h, w, c) float32 or uint8 device tensor as a
  contiguous 4-d stack, with its vtc_dtype code."""
  if torch.is_tensor(image) and image.dtype == torch.uint8:
    x = vtc_hip.require_device_tensor(image, name, torch.uint8)
    code = vtc_hip.DTYPE_U8
  else:
    x = vtc_hip.require_device_tensor(image, name)
    code = vtc_hip.DTYPE_F32
  assert x.dim() in (3, 4), 'expected (h, w, c) or (count, h, w, c)'
  assert x.numel() > 0, '%s is empty' % name
  stacked = (x if x.dim() == 4 else x[None]).contiguous()
  return stacked, code


def _device_filter(values, dtype, device, name):
  """A numpy array or tensor as a contiguous `dtype` tensor on `device`."""
  if not torch.is_tensor(values):
    values = torch.from_numpy(np.ascontiguousarray(np.asarray(values)))
  if values.is_complex() and not dtype.is_complex:
    raise TypeError('%s must be real' % name)
  return values.to(device=device).to(dtype).contiguous()


# ---- host-side filter builders (numpy in, numpy out, as in the reference) ---
def _frequency_magnitudes(DFT_num_samples):
  freqs_vert = np.fft.fftfreq(DFT_num_samples[0])
  freqs_horz = np.fft.fftfreq(DFT_num_samples[1])
  return np.sqrt(np.square(freqs_vert)[:, None] +
                 np.square(freqs_horz)[None, :])


def get_low_pass_filter(DFT_num_samples, filter_parameters,
                        norm_and_threshold=True):
  """The reference's get_low_pass_filter (image_processing.py:173-231): the
  complex128 DFT, (DFT_num_samples[0], DFT_num_samples[1]), of the zero-phase
  'exponential' low-pass exp(-(|f| / (0.5 cutoff))^order), floored at 1e-3
  when norm_and_threshold."""
  if filter_parameters['shape'] != 'exponential':
    raise KeyError('Unrecognized filter shape: ' + filter_parameters['shape'])
  assert all([x in filter_parameters for x in ['cutoff', 'order']])
  assert 0.0 <= filter_parameters['cutoff'] <= 1.0
  assert filter_parameters['order'] >= 1.0
  magnitude = np.exp(-1. * np.power(
      _frequency_magnitudes(DFT_num_samples) /
      (0.5 * filter_parameters['cutoff']), filter_parameters['order']))
  if norm_and_threshold:
    magnitude[magnitude < 1e-3] = 1e-3
  return magnitude.astype(np.complex128)


def get_whitening_ramp_filter(DFT_num_samples, norm_and_threshold=True):
  """The reference's get_whitening_ramp_filter (:234-264): the complex128 DFT
  of the zero-phase ramp |f|; norm_and_threshold divides it by its maximum
  and floors it at 1e-5."""
  magnitude = _frequency_magnitudes(DFT_num_samples)
  if norm_and_threshold:
    magnitude = magnitude / np.max(magnitude)
    magnitude[magnitude < 1e-5] = 1e-5
  return magnitude.astype(np.complex128)


def get_binomial_filter_1d(size):
  """The reference's get_binomial_filter_1d (:117-125): `size` binomial
  coefficients, normalised to sum 1."""
  assert size > 1
  kernel = np.array([0.5, 0.5])
  for _ in range(size - 2):
    kernel = np.convolve(np.array([0.5, 0.5]), kernel)
  return kernel


def get_binomial_filter_2d(height, width):
  """The reference's get_binomial_filter_2d (:128-133), for filter_sd."""
  return (get_binomial_filter_1d(height)[:, None] *
          get_binomial_filter_1d(width)[None, :])


def get_gaussian_filter_2d(sigma, window_size, normalized=True):
  """The reference's get_gaussian_filter_2d (:136-170): coordinates
  -floor(ws / 2) .. floor(ws / 2) (one fewer at the top for an even window)
  along each axis."""
  coords = []
  for size in window_size[:2]:
    half = int(np.floor(size / 2))
    coords.append(np.arange(-half, half + 1 if size % 2 != 0 else half))
  kernel = np.exp(-0.5 * (coords[0][:, None]**2 + coords[1][None, :]**2) /
                  (sigma**2))
  return kernel / np.sum(kernel) if normalized else kernel


def center_surround_filter(shape, cutoffs, norm_and_threshold=True):
  """The combined transfer function whiten_center_surround applies to an image
  of `shape` = (h, w, ...) -- what the reference hands back with
  return_filter=True (:296-304): rolled-off ramp max(|f|, low) times the
  order-8 exponential low-pass at `high`, divided by its maximum and floored
  at 1e-3 when norm_and_threshold.  Host side, complex128 (h, w); pass it to
  unwhiten_center_surround(orig_filter_DFT=...)."""
  lpf = get_low_pass_filter(
      shape, {'shape': 'exponential', 'cutoff': cutoffs['high'],
              'order': 8.0}, norm_and_threshold=False)
  wf = get_whitening_ramp_filter(shape, norm_and_threshold=False)
  combined = np.maximum(wf.real, cutoffs['low']) * lpf
  if norm_and_threshold:
    combined /= np.max(np.abs(combined))
    combined[np.abs(combined) < 1e-3] = 1e-3
  return combined


# ---- filters ---------------------------------------------------------------------
def filter_fd(image, filter_DFT):
  """
  The reference's filter_fd (image_processing.py:63-92) on the device.

  image : float32 or uint8 tensor on a HIP device, (h, w, c) or a stack
      (count, h, w, c).
  filter_DFT : (fh, fw) complex128 (or real) numpy array or device tensor,
      fh >= h and fw >= w; any complex values, no symmetry assumed.
  Returns real(ifft2(filter_DFT * fft2(image, (fh, fw))))[:h, :w] per channel,
  float64 transforms rounded once to float32.
  """
  lib = vtc_hip.load_library()
  stacked, code = _image_input(image, 'image')
  count, h, w, c = stacked.shape
  filt = _device_filter(filter_DFT, torch.complex128, stacked.device,
                        'filter_DFT')
  assert filt.dim() == 2, 'filter_DFT must be (fh, fw)'
  fh, fw = filt.shape
  assert fh >= h, "don't undersample DFT"
  assert fw >= w, "don't undersample DFT"
  out = torch.empty(stacked.shape, dtype=torch.float32, device=stacked.device)
  ws = vtc_hip.workspace(
      lib.vtc_img_filter_fd_workspace_bytes(count, h, w, c, fh, fw),
      stacked.device)
  vtc_hip.check(lib.vtc_img_filter_fd(
      vtc_hip.ptr(stacked), code, vtc_hip.ptr(filt), vtc_hip.ptr(out), count,
      h, w, c, fh, fw, vtc_hip.ptr(ws), ws.numel(),
      vtc_hip.current_stream(stacked.device)), 'vtc_img_filter_fd')
  return out if image.dim() == 4 else out[0]


def filter_sd(image, filter_spatial, separable_vert=None, separable_horz=None):
  """
  The reference's filter_sd (image_processing.py:18-60) on the device.

  image : float32 or uint8 tensor on a HIP device, (h, w, c) or a stack.
  filter_spatial : (fh, fw) numpy array or device tensor (used as float64).
  separable_vert, separable_horz : the (fh,) and (fw,) factors; when given
      (both), the two 1-d 'reflect' convolutions of the reference run instead,
      the horizontal one first, its result stored in the image's own element
      type as scipy does, and filter_spatial is not read.
  Without them: scipy's convolve2d(..., 'same', boundary='symm') per channel.
  Float64 sums, float32 result.  A filter larger than the image in either
  axis or with more than 63 taps per axis raises NotImplementedError.
  """
  lib = vtc_hip.load_library()
  stacked, code = _image_input(image, 'image')
  count, h, w, c = stacked.shape
  device = stacked.device
  separable = separable_vert is not None
  if separable:
    assert separable_horz is not None, 'both separable factors are needed'
    vert = _device_filter(separable_vert, torch.float64, device,
                          'separable_vert').reshape(-1)
    horz = _device_filter(separable_horz, torch.float64, device,
                          'separable_horz').reshape(-1)
    filt, fh, fw = None, vert.numel(), horz.numel()
  else:
    filt = _device_filter(filter_spatial, torch.float64, device,
                          'filter_spatial')
    assert filt.dim() == 2, 'filter_spatial must be (fh, fw)'
    vert, horz, (fh, fw) = None, None, filt.shape
  out = torch.empty(stacked.shape, dtype=torch.float32, device=device)
  ws = vtc_hip.workspace(lib.vtc_img_filter_sd_workspace_bytes(
      count, h, w, c, fh, fw, 1 if separable else 0), device)
  vtc_hip.check(lib.vtc_img_filter_sd(
      vtc_hip.ptr(stacked), code, vtc_hip.ptr(filt), vtc_hip.ptr(vert),
      vtc_hip.ptr(horz), vtc_hip.ptr(out), count, h, w, c, fh, fw,
      vtc_hip.ptr(ws), ws.numel(), vtc_hip.current_stream(device)),
      'vtc_img_filter_sd')
  return out if image.dim() == 4 else out[0]


def downsample(image, factor=2):
  """The reference's downsample (image_processing.py:95-114) on the device:
  image[::factor, ::factor] of a (h, w, c) image, or of every image of a
  (count, h, w, c) stack, as a new tensor of the same element type."""
  assert type(factor) == int
  assert factor >= 1
  stacked, code = _image_input(image, 'image')
  count, h, w, c = stacked.shape
  out = torch.empty((count, -(-h // factor), -(-w // factor), c),
                    dtype=stacked.dtype, device=stacked.device)
  vtc_hip.check(vtc_hip.load_library().vtc_img_downsample(
      vtc_hip.ptr(stacked), code, vtc_hip.ptr(out), count, h, w, c, factor,
      vtc_hip.current_stream(stacked.device)), 'vtc_img_downsample')
  return out if image.dim() == 4 else out[0]


# ---- tiling ------------------------------------------------------------------------
def patches_from_single_image(image, patch_dimensions, flatten_patches):
  """
  The reference's patches_from_single_image (image_processing.py:597-648) on
  the device.

  image : float32 or uint8 device tensor (h, w, c), or a stack
      (count, h, w, c) (an extension: the patch axis then follows the image
      axis).
  Returns (patches, patch_positions): the k = (h // ph) * (w // pw) tiled
  patches, (k, ph, pw, c) or flattened (k, ph*pw*c), element type kept, and
  the reference's host list of (row, column) corners.  Prints the reference's
  warning when the image does not tile exactly.
  """
  stacked, code = _image_input(image, 'image')
  count, h, w, c = stacked.shape
  ph, pw = int(patch_dimensions[0]), int(patch_dimensions[1])
  if h / ph % 1 != 0 or w / pw % 1 != 0:
    print('Warning: image cannot be completely patched with these dimensions.',
          'Ignoring overflow pixels on the right and bottom of image')
  num_vert, num_horz = h // ph, w // pw
  patches = torch.empty((count, num_vert * num_horz, ph, pw, c),
                        dtype=stacked.dtype, device=stacked.device)
  if patches.numel():
    vtc_hip.check(vtc_hip.load_library().vtc_img_tile_patches(
        vtc_hip.ptr(stacked), code, vtc_hip.ptr(patches), count, h, w, c, ph,
        pw, vtc_hip.current_stream(stacked.device)), 'vtc_img_tile_patches')
  patch_positions = [(i * ph, j * pw) for i in range(num_vert)
                     for j in range(num_horz)]
  if flatten_patches:
    patches = patches.reshape(count, num_vert * num_horz, -1)
  return (patches if image.dim() == 4 else patches[0]), patch_positions


def _positions_disjoint(positions, ph, pw, height, width):
  """True when no two (ph, pw) patches at `positions` (k, 2) overlap: a 2-d
  difference array counts the patches over every pixel."""
  cover = np.zeros((height + 1, width + 1), dtype=np.int64)
  v, u = positions[:, 0], positions[:, 1]
  np.add.at(cover, (v, u), 1)
  np.add.at(cover, (v + ph, u), -1)
  np.add.at(cover, (v, u + pw), -1)
  np.add.at(cover, (v + ph, u + pw), 1)
  return int(cover.cumsum(axis=0).cumsum(axis=1).max()) <= 1


def assemble_image_from_patches(patches, patch_dimensions, patch_positions):
  """
  The reference's assemble_image_from_patches (image_processing.py:651-699)
  on the device.

  patches : float32 or uint8 device tensor, (k, ph*pw*c) or (k, ph, pw, c).
  patch_positions : k (row, column) corners in the order of `patches` (any
      order, any subset; the host list patches_from_single_image returns).
  Returns the (max row + ph, max column + pw, c) image, zeros where no patch
  lies; where patches overlap the later one is kept, as in the reference.
  """
  if torch.is_tensor(patches) and patches.dtype == torch.uint8:
    x = vtc_hip.require_device_tensor(patches, 'patches', torch.uint8)
    code = vtc_hip.DTYPE_U8
  else:
    x = vtc_hip.require_device_tensor(patches, 'patches')
    code = vtc_hip.DTYPE_F32
  assert x.dim() in (2, 4), 'expected (k, ph*pw*c) or (k, ph, pw, c)'
  ph, pw = int(patch_dimensions[0]), int(patch_dimensions[1])
  positions = np.asarray(patch_positions, dtype=np.int64).reshape(-1, 2)
  k = x.shape[0]
  assert k > 0 and positions.shape[0] == k, 'one position per patch'
  assert positions.min() >= 0, 'negative patch position'
  height = int(positions[:, 0].max()) + ph
  width = int(positions[:, 1].max()) + pw
  if x.dim() == 2:
    channels = x.shape[1] / (ph * pw)
    assert channels % 1.0 == 0
    channels = int(channels)
  else:
    assert x.shape[1:3] == (ph, pw), 'patches do not match patch_dimensions'
    channels = x.shape[-1]
  x = x.contiguous()
  table = torch.from_numpy(positions.astype(np.int32)).to(x.device)
  image = torch.empty((height, width, channels), dtype=x.dtype,
                      device=x.device)
  vtc_hip.check(vtc_hip.load_library().vtc_img_assemble_patches(
      vtc_hip.ptr(x), code, vtc_hip.ptr(table), vtc_hip.ptr(image), k, ph, pw,
      channels, height, width,
      1 if _positions_disjoint(positions, ph, pw, height, width) else 0,
      vtc_hip.current_stream(x.device)), 'vtc_img_assemble_patches')
  return image


def unwhiten_center_surround(image, low_cutoff=None, orig_filter_DFT=None):
  """
  The reference's unwhiten_center_surround (image_processing.py:311-335) on
  the device: filter_fd(image, 1 / F).

  image : float32 device tensor, (h, w, c) or a stack.
  orig_filter_DFT : the (h, w) transfer function the image was whitened with
      (center_surround_filter gives it), numpy array or device tensor: the
      whitening is inverted exactly.
  low_cutoff : used when orig_filter_DFT is None: F = max(|f|, low_cutoff),
      the rolled-off ramp without the low-pass, whose inverse would amplify
      noise.
  """
  assert torch.is_tensor(image) and image.dtype == torch.float32
  assert not ((low_cutoff is None) and (orig_filter_DFT is None))
  if orig_filter_DFT is None:
    shape = image.shape[-3:]
    wf = get_whitening_ramp_filter(shape, norm_and_threshold=False)
    orig_filter_DFT = np.maximum(wf.real, low_cutoff).astype(np.complex128)
  if torch.is_tensor(orig_filter_DFT):
    inverse = torch.reciprocal(orig_filter_DFT.to(torch.complex128))
  else:
    inverse = 1. / np.asarray(orig_filter_DFT)
  return filter_fd(image, inverse)
