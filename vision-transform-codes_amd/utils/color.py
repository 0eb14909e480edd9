"""
Colour on the device: RGB <-> YCbCr (or any 3 x 3 colour basis), chroma planes
at reduced resolution and back, and one point of a rate-distortion curve for a
colour image -- three planes coded with luma and chroma tables, decoded from
the bytes, merged and measured on the image.

The reference has no colour path (its dataset_generation.py:149-150 leaves
'Kodak' at "This is next"); this module is the extension, built on the kernels
of csrc/color.hip behind include/ext/vtc_color.h and on what utils.jpeg,
utils.image_processing and utils.plotting already have.  DESIGN.md 4.22 states
the arithmetic: float64 operations in a fixed order, one rounding to float32.

Images are float32 device tensors, (h, w, 3) or (count, h, w, 3) ('hwc', the
layout of the training-set builder) or (3, h, w) / (count, 3, h, w) ('chw',
the layout of the convolutional engine); planes are (h, w) or (count, h, w).
A wrong shape raises ValueError, then a CPU tensor VtcHipError.
"""
import ctypes
import pickle

import numpy as np
import torch

import vtc_hip

# JFIF 1.02, the ten decimal constants.  Rows of JFIF_FORWARD give Y, Cb, Cr
# from R, G, B; rows of JFIF_INVERSE give R, G, B from Y, Cb - o, Cr - o.
JFIF_FORWARD = ((0.299, 0.587, 0.114),
                (-0.168736, -0.331264, 0.5),
                (0.5, -0.418688, -0.081312))
JFIF_INVERSE = ((1.0, 0.0, 1.402),
                (1.0, -0.344136, -0.714136),
                (1.0, 1.772, 0.0))

LAYOUTS = {'hwc': vtc_hip.COLOR_HWC, 'chw': vtc_hip.COLOR_CHW}
UPSAMPLING = {'replicate': vtc_hip.UPSAMPLE_REPLICATE,
              'triangle': vtc_hip.UPSAMPLE_TRIANGLE}
FACTORS = (1, 2, 4)


# ----------------------------------------------------------------- arguments
def _layout(name, what):
  if name not in LAYOUTS:
    raise ValueError("%s must be 'hwc' or 'chw', got %r" % (what, name))
  return LAYOUTS[name]


def _shape_of(t, name):
  if not torch.is_tensor(t):
    raise TypeError('%s must be a torch.Tensor' % name)
  return tuple(int(v) for v in t.shape)


def _image_stack(images, layout, name='images'):
  """(contiguous 4-d stack, count, h, w, stacked?) of an image or a stack in
  `layout`; the shape is judged before the device."""
  shape = _shape_of(images, name)
  axis = -1 if layout == 'hwc' else -3
  if len(shape) not in (3, 4) or shape[axis] != 3 or 0 in shape:
    raise ValueError(
        '%s must be %s, got shape %s' % (
            name, '(h, w, 3) or (count, h, w, 3)' if layout == 'hwc' else
            '(3, h, w) or (count, 3, h, w)', shape))
  x = vtc_hip.require_device_tensor(images, name)
  stacked = (x if x.dim() == 4 else x[None]).contiguous()
  if layout == 'hwc':
    count, h, w, _ = stacked.shape
  else:
    count, _, h, w = stacked.shape
  return stacked, count, h, w, x.dim() == 4


def _plane_stack(planes, name='planes'):
  shape = _shape_of(planes, name)
  if len(shape) not in (2, 3) or 0 in shape:
    raise ValueError('%s must be (h, w) or (count, h, w), got shape %s'
                     % (name, shape))
  x = vtc_hip.require_device_tensor(planes, name)
  return (x if x.dim() == 3 else x[None]).contiguous(), x.dim() == 3


def _factors(factors):
  try:
    fv, fh = (int(f) for f in factors)
  except (TypeError, ValueError):
    raise ValueError('factors must be (vertical, horizontal), got %r'
                     % (factors,))
  for f in (fv, fh):
    if f not in FACTORS:
      raise ValueError('subsampling factors are 1, 2 or 4, got %r'
                       % (factors,))
  return fv, fh


def _three(values, name):
  if values is None:
    return (ctypes.c_double * 3)(0.0, 0.0, 0.0)
  values = np.asarray(values, dtype=np.float64).reshape(-1)
  if values.shape[0] != 3:
    raise ValueError('%s must have 3 entries, got %d' % (name,
                                                         values.shape[0]))
  return (ctypes.c_double * 3)(*values.tolist())


def _clamp(clamp):
  if clamp is None:
    return 0, 0.0, 0.0
  try:
    lo, hi = (float(v) for v in clamp)
  except (TypeError, ValueError):
    raise ValueError('clamp must be None or (lo, hi), got %r' % (clamp,))
  if not lo <= hi:
    raise ValueError('clamp needs lo <= hi, got %r' % (clamp,))
  return 1, lo, hi


# ------------------------------------------------------------- device calls
def color_transform(images, matrix, pre=None, post=None, clamp=None,
                    layout='hwc', out_layout=None):
  """out_i = ((m_i0 t_0 + m_i1 t_1) + m_i2 t_2) + post_i with t_j = in_j -
  pre_j, per pixel, in float64, then clamped to clamp = (lo, hi) when given (a
  NaN stays a NaN) and rounded once to float32.

  images : float32 device tensor in `layout`
  matrix : 3 x 3 host numbers, row-major; pre, post : 3 host numbers or None
  layout, out_layout : 'hwc' or 'chw'; out_layout None keeps `layout`

  Returns a new tensor in out_layout, a stack when `images` is one.  The same
  call does forward JFIF, inverse JFIF or a learned colour basis such as PCA
  axes.
  """
  out_layout = layout if out_layout is None else out_layout
  in_code, out_code = _layout(layout, 'layout'), _layout(out_layout,
                                                         'out_layout')
  m = np.asarray(matrix, dtype=np.float64)
  if m.size != 9:
    raise ValueError('matrix must be 3 x 3, got shape %s' % (m.shape,))
  m = (ctypes.c_double * 9)(*m.reshape(-1).tolist())
  pre, post = _three(pre, 'pre'), _three(post, 'post')
  flag, lo, hi = _clamp(clamp)
  stacked, count, h, w, is_stack = _image_stack(images, layout)
  shape = (count, h, w, 3) if out_layout == 'hwc' else (count, 3, h, w)
  out = torch.empty(shape, dtype=torch.float32, device=stacked.device)
  vtc_hip.check(vtc_hip.load_library().vtc_color_transform(
      vtc_hip.ptr(stacked), in_code, vtc_hip.ptr(out), out_code, count, h, w,
      ctypes.cast(m, ctypes.c_void_p), ctypes.cast(pre, ctypes.c_void_p),
      ctypes.cast(post, ctypes.c_void_p), flag, lo, hi,
      vtc_hip.current_stream(stacked.device)), 'vtc_color_transform')
  return out if is_stack else out[0]


def rgb_to_ycbcr(images, chroma_offset=128.0, layout='hwc', out_layout=None):
  """JFIF YCbCr of RGB images: color_transform with JFIF_FORWARD and post =
  (0, o, o).  chroma_offset o is 128 for data in [0, 255] and 0.5 for data in
  [0, 1].  A grey pixel R = G = B of an 8-bit level gives Y = that level and
  Cb = Cr = o exactly."""
  o = float(chroma_offset)
  return color_transform(images, JFIF_FORWARD, post=(0.0, o, o), layout=layout,
                         out_layout=out_layout)


def ycbcr_to_rgb(images, chroma_offset=128.0, clamp=None, layout='hwc',
                 out_layout=None):
  """RGB of JFIF YCbCr images: color_transform with JFIF_INVERSE and pre =
  (0, o, o), clamped to clamp = (lo, hi) when given."""
  o = float(chroma_offset)
  return color_transform(images, JFIF_INVERSE, pre=(0.0, o, o), clamp=clamp,
                         layout=layout, out_layout=out_layout)


def subsample_plane(planes, factors):
  """Box mean: (h, w) or (count, h, w) float32 planes to ceil(h / fv) x
  ceil(w / fh), factors = (fv, fh) each 1, 2 or 4.  A ragged edge averages the
  pixels that exist."""
  fv, fh = _factors(factors)
  stacked, is_stack = _plane_stack(planes)
  count, h, w = stacked.shape
  out = torch.empty((count, -(-h // fv), -(-w // fh)), dtype=torch.float32,
                    device=stacked.device)
  vtc_hip.check(vtc_hip.load_library().vtc_plane_downsample(
      vtc_hip.ptr(stacked), vtc_hip.ptr(out), count, h, w, fv, fh,
      vtc_hip.current_stream(stacked.device)), 'vtc_plane_downsample')
  return out if is_stack else out[0]


def upsample_plane(planes, factors, shape, mode='triangle'):
  """Reduced planes back to shape = (h, w), where ceil(h / fv) and
  ceil(w / fh) are the planes' sides.  mode 'replicate' repeats every pixel,
  'triangle' interpolates linearly between pixel centres, clamped at the edge
  (for a factor of 2 libjpeg's 3/4, 1/4 weights)."""
  fv, fh = _factors(factors)
  if mode not in UPSAMPLING:
    raise ValueError("mode must be 'replicate' or 'triangle', got %r"
                     % (mode,))
  try:
    h, w = (int(v) for v in shape)
  except (TypeError, ValueError):
    raise ValueError('shape must be (h, w), got %r' % (shape,))
  got = _shape_of(planes, 'planes')
  if h < 1 or w < 1 or got[-2:] != (-(-h // fv), -(-w // fh)):
    raise ValueError(
        'planes of shape %s do not upsample by %s to %s'
        % (got, (fv, fh), (h, w)))
  stacked, is_stack = _plane_stack(planes)
  count, h_in, w_in = stacked.shape
  out = torch.empty((count, h, w), dtype=torch.float32, device=stacked.device)
  vtc_hip.check(vtc_hip.load_library().vtc_plane_upsample(
      vtc_hip.ptr(stacked), vtc_hip.ptr(out), count, h_in, w_in, h, w, fv, fh,
      UPSAMPLING[mode], vtc_hip.current_stream(stacked.device)),
                'vtc_plane_upsample')
  return out if is_stack else out[0]


# ------------------------------------------------------------------- planes
def split_planes(image, subsampling=(2, 2), chroma_offset=128.0):
  """[Y, Cb, Cr] of one (h, w, 3) RGB image: Y (h, w), Cb and Cr at
  ceil(h / fv) x ceil(w / fh), subsampling = (fv, fh).  Each plane can then go
  through a single-channel route (utils.jpeg, utils.quantization,
  utils.vector_quantization) as it is."""
  shape = _shape_of(image, 'image')
  if len(shape) != 3 or shape[2] != 3 or 0 in shape:
    raise ValueError('image must be (h, w, 3), got shape %s' % (shape,))
  factors = _factors(subsampling)
  ycc = rgb_to_ycbcr(image, chroma_offset, out_layout='chw')
  chroma = subsample_plane(ycc[1:], factors)
  return [ycc[0], chroma[0], chroma[1]]


def merge_planes(planes, shape, subsampling=(2, 2), chroma_offset=128.0,
                 upsampling='triangle', clamp=None):
  """The (h, w, 3) RGB image of [Y, Cb, Cr] as split_planes lays them out:
  shape = (h, w), the chroma planes upsampled by `upsampling`, then
  ycbcr_to_rgb with `clamp`."""
  if len(planes) != 3:
    raise ValueError('planes must be [Y, Cb, Cr]')
  factors = _factors(subsampling)
  try:
    h, w = (int(v) for v in shape)
  except (TypeError, ValueError):
    raise ValueError('shape must be (h, w), got %r' % (shape,))
  luma, cb, cr = planes
  if _shape_of(luma, 'Y') != (h, w):
    raise ValueError('Y must be %s, got shape %s' % ((h, w), tuple(luma.shape)))
  if _shape_of(cb, 'Cb') != _shape_of(cr, 'Cr'):
    raise ValueError('Cb and Cr must have one shape')
  for t, name in ((luma, 'Y'), (cb, 'Cb'), (cr, 'Cr')):
    vtc_hip.require_device_tensor(t, name)
  ycc = torch.empty((3, h, w), dtype=torch.float32, device=luma.device)
  ycc[0] = luma
  ycc[1:] = upsample_plane(torch.stack([cb, cr]), factors, (h, w), upsampling)
  return ycbcr_to_rgb(ycc, chroma_offset, clamp, layout='chw',
                      out_layout='hwc')


# ------------------------------------------------------------------ loaders
def load_kodak(filepath):
  """The colour Kodak set: a pickled list of (h, w, 3) uint8 arrays, read
  through the restricted unpickler of training.sparse_coding (a file that
  names anything but plain numpy arrays raises pickle.UnpicklingError).
  Returns a list of float32 (h, w, 3) arrays, which
  dataset_generation.create_patch_training_set takes as `dataset`."""
  from training.sparse_coding import _ArrayUnpickler
  with open(filepath, 'rb') as f:
    raw = _ArrayUnpickler(f).load()
  if not isinstance(raw, (list, tuple)):
    raise pickle.UnpicklingError('Kodak: expected a list of arrays')
  images = []
  for x in raw:
    x = np.asarray(x)
    if x.ndim != 3 or x.shape[2] != 3:
      raise ValueError('Kodak: expected (h, w, 3) arrays, got shape %s'
                       % (x.shape,))
    images.append(x.astype('float32'))
  return images


# ------------------------------------------------------------ the R-D point
def _plane_levels(plane, dictionary, patch_dimensions, widths, order, shift):
  """(levels, patch positions, shift vector or None) of one plane: tiled,
  level-shifted, analysed and quantised as utils.jpeg.rate_distortion_image
  does."""
  from analysis_transforms.fully_connected import invertible_linear
  from utils import image_processing, jpeg
  patches, positions = image_processing.patches_from_single_image(
      plane[:, :, None], patch_dimensions, flatten_patches=True)
  means = None
  if shift is not None:
    means = torch.full((patches.shape[1],), shift, dtype=torch.float32,
                       device=plane.device)
    patches = image_processing._column_apply(
        patches, vtc_hip.DTYPE_F32, vtc_hip.COLUMN_SUBTRACT, means)
  levels = jpeg.quantize(invertible_linear.run(patches, dictionary), widths,
                         order)
  return levels, positions, means


def rate_distortion_image_color(image, dictionary, patch_dimensions,
                                luma_binwidths, chroma_binwidths,
                                quant_multiplier, subsampling=(2, 2),
                                tables=None, order=None, chroma_offset=128.0,
                                level_shift=None, upsampling='triangle',
                                clamp=None, signal_magnitude=255.0,
                                chroma_dictionary=None):
  """One point of a rate-distortion curve for a colour image, the way baseline
  JPEG lays a colour image out.

  image : (h, w, 3) float32 RGB device tensor.  It is cropped to whole MCUs,
      H = h // (ph fv) * (ph fv) and W = w // (pw fh) * (pw fh); pixels beyond
      are left out of every figure, as utils.jpeg.rate_distortion_image leaves
      out partial patches.
  dictionary : (n, n) float32 device tensor, n = ph * pw, for all three planes
      unless chroma_dictionary gives Cb and Cr one of their own
  luma_binwidths, chroma_binwidths : n floats in scan order; the bins used are
      these times quant_multiplier
  subsampling : (fv, fh) of the chroma planes, each 1, 2 or 4
  tables : ((ac, dc) luma, (ac, dc) chroma), or None to train the luma pair on
      Y's symbol counts and the chroma pair on the sum of Cb's and Cr's, which
      share a pair as in JPEG
  order : scan order of the code columns, or None
  level_shift : None or a number subtracted from every sample of every plane
      before analysis and added back after decoding (JPEG's 128)
  upsampling, clamp : how merge_planes brings the decoded planes back to RGB
  signal_magnitude : the range pSNR and SSIM are measured against

  Every plane is tiled, shifted, analysed (invertible_linear), quantised,
  packed into its JPEG streams, decoded from those bytes (decode_patches) and
  reassembled.  Returns a dict: 'bits' (Y, Cb, Cr stream bits, ints),
  'bits_per_pixel' (their sum over H W), 'pSNR' (compute_pSNR of the (H, W, 3)
  RGB pair), 'pSNR_Y' and 'SSIM_Y' (of the Y pair), 'tables' and
  'reconstruction' (the (H, W, 3) device tensor).
  """
  from utils import image_processing, jpeg, plotting
  shape = _shape_of(image, 'image')
  if len(shape) != 3 or shape[2] != 3:
    raise ValueError('image must be (h, w, 3), got shape %s' % (shape,))
  fv, fh = _factors(subsampling)
  ph, pw = int(patch_dimensions[0]), int(patch_dimensions[1])
  H = shape[0] // (ph * fv) * (ph * fv)
  W = shape[1] // (pw * fh) * (pw * fh)
  if H == 0 or W == 0:
    raise ValueError('image %s holds no %d x %d unit (patches of %d x %d at '
                     'subsampling %s)' % (shape, ph * fv, pw * fh, ph, pw,
                                          (fv, fh)))
  image = vtc_hip.require_device_tensor(image, 'image')
  dictionary = vtc_hip.require_device_tensor(dictionary, 'dictionary')
  if chroma_dictionary is None:
    chroma_dictionary = dictionary
  else:
    chroma_dictionary = vtc_hip.require_device_tensor(chroma_dictionary,
                                                      'chroma_dictionary')
  shift = None if level_shift is None else float(level_shift)
  original = image[:H, :W].contiguous()
  planes = split_planes(original, (fv, fh), chroma_offset)
  dictionaries = (dictionary, chroma_dictionary, chroma_dictionary)
  binwidths = (luma_binwidths, chroma_binwidths, chroma_binwidths)
  coded = []
  for plane, d, widths in zip(planes, dictionaries, binwidths):
    scaled = np.asarray(widths, dtype=np.float64) * quant_multiplier
    coded.append(_plane_levels(plane, d, (ph, pw), scaled, order, shift))
  if tables is None:
    counts = [jpeg.symbol_counts(levels) for levels, _, _ in coded]
    tables = (jpeg.tables_from_counts(*counts[0]),
              jpeg.tables_from_counts(counts[1][0] + counts[2][0],
                                      counts[1][1] + counts[2][1]))
  bits, decoded = [], []
  for (levels, positions, means), d, widths, pair in zip(
      coded, dictionaries, binwidths, (tables[0], tables[1], tables[1])):
    packed, offsets = jpeg.pack_streams(levels, pair[0], pair[1])
    bits.append(int(offsets[-1]))
    back = jpeg.decode_patches(packed, offsets, d, widths, quant_multiplier,
                               pair, order)
    if means is not None:   # x - (-m): the addition, in float32
      back = image_processing._column_apply(
          back, vtc_hip.DTYPE_F32, vtc_hip.COLUMN_SUBTRACT, -means)
    decoded.append(image_processing.assemble_image_from_patches(
        back, (ph, pw), positions)[:, :, 0])
  reconstruction = merge_planes(decoded, (H, W), (fv, fh), chroma_offset,
                                upsampling, clamp)
  return {'bits': tuple(bits),
          'bits_per_pixel': sum(bits) / float(H * W),
          'pSNR': plotting.compute_pSNR(original, reconstruction,
                                        manual_sig_mag=signal_magnitude),
          'pSNR_Y': plotting.compute_pSNR(planes[0], decoded[0],
                                          manual_sig_mag=signal_magnitude),
          'SSIM_Y': plotting.compute_ssim(planes[0], decoded[0],
                                          manual_sig_mag=signal_magnitude),
          'tables': tables,
          'reconstruction': reconstruction}
