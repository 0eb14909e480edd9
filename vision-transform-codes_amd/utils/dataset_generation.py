"""
The patch pipeline of utils/dataset_generation.py on MI355X: range
standardisation (:169-183), patch positions (:205-214) and extraction
(:184-222).  Images stay in HBM; the positions come from the caller's numpy
generator in the reference's order (image index, vertical, horizontal per
patch), so a seeded run selects the same patches.

create_patch_training_set (:22-311) runs every preprocessing op of the
reference on the device, in the caller's order.
"""
import ctypes
import pickle

import numpy as np
import torch

import vtc_hip
from utils import image_processing as ip_util


class OneOutputDset(torch.utils.data.Dataset):
  """Just like torch.utils.data.TensorDataset, but doesn't return a tuple
  (dataset_generation.py:13-20)."""
  def __init__(self, single_tensor):
    self.tensor = single_tensor

  def __getitem__(self, index):
    return self.tensor[index]

  def __len__(self):
    return self.tensor.size(0)


def standardize_data_range(images):
  """(images - min) / (max - min) over the whole stack, float32 like numpy's
  (dataset_generation.py:169-183; asserts max > min as the reference does).
  images: float32 tensor of any shape on a HIP device; returns a new tensor."""
  lib = vtc_hip.load_library()
  images = vtc_hip.require_device_tensor(images, 'images').contiguous()
  out = torch.empty_like(images)
  min_max = torch.empty(2, dtype=torch.float32, device=images.device)
  ws = vtc_hip.workspace(lib.vtc_window_minmax_workspace_bytes(),
                         images.device)
  vtc_hip.check(lib.vtc_standardize_data_range(
      vtc_hip.ptr(images), vtc_hip.ptr(out), images.numel(),
      vtc_hip.ptr(min_max), vtc_hip.ptr(ws), ws.numel(),
      vtc_hip.current_stream(images.device)), 'vtc_standardize_data_range')
  lo, hi = min_max.tolist()
  assert hi > lo
  return out


def _position_limits(image_shape, patch_dimensions, edge_buffer, num_images):
  shapes = [tuple(image_shape)[:2]] * num_images if np.isscalar(
      image_shape[0]) else [tuple(x)[:2] for x in image_shape]
  assert len(shapes) == num_images
  max_vert = [x[0] - patch_dimensions[0] - edge_buffer for x in shapes]
  max_horz = [x[1] - patch_dimensions[1] - edge_buffer for x in shapes]
  return max_vert, max_horz


def draw_patch_positions_loop(num_samples, image_shape, patch_dimensions,
                              edge_buffer, num_images, rng=np.random):
  """The reference's loop as it stands: three randint calls per patch
  (dataset_generation.py:205-214).  Kept as the statement of what
  draw_patch_positions must reproduce (tests/test_host_logic.py) and for
  generators that are not numpy's legacy RandomState."""
  max_vert, max_horz = _position_limits(image_shape, patch_dimensions,
                                        edge_buffer, num_images)
  img_idx = np.empty(num_samples, np.int32)
  vert = np.empty(num_samples, np.int32)
  horz = np.empty(num_samples, np.int32)
  for p_idx in range(num_samples):
    img_idx[p_idx] = rng.randint(low=0, high=num_images)
    vert[p_idx] = rng.randint(low=edge_buffer, high=max_vert[img_idx[p_idx]])
    horz[p_idx] = rng.randint(low=edge_buffer, high=max_horz[img_idx[p_idx]])
  return img_idx, vert, horz


def draw_patch_positions(num_samples, image_shape, patch_dimensions,
                         edge_buffer, num_images, rng=np.random):
  """The three randint values per patch of dataset_generation.py:205-214, for
  all patches in one native call (vtc_draw_patch_positions: MT19937 + randint's
  masked rejection sampling on the generator's own state, which is advanced
  exactly as the loop would advance it): 131 072 positions in ~2 ms instead of
  0.3-0.4 s of interpreter time.  image_shape: one (h, w) for equally sized
  images, or a sequence of num_images shapes -- the reference keeps per-image
  position ranges (:185-198).  rng: numpy.random (the global legacy generator)
  or a numpy.random.RandomState; anything else takes the loop.  Returns int32
  arrays (img_idx, vert_pos, horz_pos)."""
  state_owner = rng.mtrand._rand if rng is np.random else rng
  if not isinstance(state_owner, np.random.RandomState):
    return draw_patch_positions_loop(num_samples, image_shape,
                                     patch_dimensions, edge_buffer,
                                     num_images, rng)
  max_vert, max_horz = _position_limits(image_shape, patch_dimensions,
                                        edge_buffer, num_images)
  kind, key, pos, has_gauss, cached = state_owner.get_state()
  assert kind == 'MT19937'
  key = np.ascontiguousarray(key, dtype=np.uint32).copy()
  pos_c = ctypes.c_int32(int(pos))
  mv = np.asarray(max_vert, dtype=np.int32)
  mh = np.asarray(max_horz, dtype=np.int32)
  img_idx = np.empty(num_samples, np.int32)
  vert = np.empty(num_samples, np.int32)
  horz = np.empty(num_samples, np.int32)

  def p(a):
    return ctypes.c_void_p(a.ctypes.data)
  vtc_hip.check(vtc_hip.load_library().vtc_draw_patch_positions(
      p(key), ctypes.cast(ctypes.byref(pos_c), ctypes.c_void_p),
      int(num_samples), int(num_images), int(edge_buffer), p(mv), p(mh),
      p(img_idx), p(vert), p(horz)), 'vtc_draw_patch_positions')
  state_owner.set_state((kind, key, pos_c.value, has_gauss, cached))
  return img_idx, vert, horz


def extract_patches(images, img_idx, vert_pos, horz_pos, patch_dimensions,
                    flatten=True):
  """
  images : (count, h, w, c) float32 on a HIP device.
  img_idx, vert_pos, horz_pos : integer arrays (numpy or tensors), one entry
      per patch.
  Returns (num, ph*pw*c) if flatten else (num, ph, pw, c): patch p is
  images[img_idx[p], vert:vert+ph, horz:horz+pw, :].
  """
  lib = vtc_hip.load_library()
  images = vtc_hip.require_device_tensor(images, 'images').contiguous()
  assert images.dim() == 4, 'expected (count, h, w, c)'
  count, h, w, c = images.shape
  ph, pw = int(patch_dimensions[0]), int(patch_dimensions[1])
  device = images.device

  def as_i32(a):
    a = np.asarray(a.cpu() if torch.is_tensor(a) else a)
    return torch.from_numpy(a.astype(np.int32)).to(device)

  idx_np = np.asarray(img_idx.cpu() if torch.is_tensor(img_idx) else img_idx)
  v_np = np.asarray(vert_pos.cpu() if torch.is_tensor(vert_pos) else vert_pos)
  h_np = np.asarray(horz_pos.cpu() if torch.is_tensor(horz_pos) else horz_pos)
  num = int(idx_np.shape[0])
  if num:
    if (idx_np.min() < 0 or idx_np.max() >= count or v_np.min() < 0 or
        v_np.max() + ph > h or h_np.min() < 0 or h_np.max() + pw > w):
      raise IndexError('patch position outside the image stack')
  patches = torch.empty((num, ph * pw * c), dtype=torch.float32, device=device)
  # keep the index tensors alive until the launch is enqueued
  idx_d, vert_d, horz_d = as_i32(idx_np), as_i32(v_np), as_i32(h_np)
  vtc_hip.check(lib.vtc_extract_patches(
      vtc_hip.ptr(images), vtc_hip.ptr(idx_d), vtc_hip.ptr(vert_d),
      vtc_hip.ptr(horz_d), vtc_hip.ptr(patches), num, h, w, c, ph, pw,
      vtc_hip.current_stream(device)), 'vtc_extract_patches')
  return patches if flatten else patches.reshape(num, ph, pw, c)


PREPROC_OPS = ('standardize_data_range', 'whiten_center_surround',
               'whiten_ZCA', 'patch', 'pad', 'center_each_component',
               'center_each_patch', 'normalize_component_variance',
               'local_contrast_normalization', 'local_luminance_subtraction')
DATASETS = ('Field_NW', 'vanHateren', 'Kodak_BW', 'Kodak')
_BEFORE_PATCH = {
    'whiten_center_surround': 'We typically preform this type of whitening '
                              'before patching the images',
    'local_contrast_normalization': 'We typically preform this before '
                                    'patching the images',
    'local_luminance_subtraction': 'We typically preform this before '
                                   'patching the images'}
_AFTER_PATCH = {
    'whiten_ZCA': 'You ought to patch image before trying to compute a ZCA '
                  'whitening transform',
    'center_each_component': 'You ought to patch the data before trying to '
                             'center each component',
    'normalize_component_variance': 'You ought to patch the data before '
                                    'normalizing it',
    'center_each_patch': 'You ought to patch the data before trying to '
                         'center each patch',
    'pad': 'You ought to patch the data first. Padding is added to the '
           'patches'}


def check_request(dataset, order_of_preproc_ops, extra_params):
  """Every error create_patch_training_set can raise from its arguments
  alone, with the reference's exception types (dataset_generation.py:93-103,
  :130-131 and the op loop :162-282), in the order the reference would meet
  them.  Host only: nothing is read and no device is touched."""
  ops = list(order_of_preproc_ops)
  assert 'patch' in ops
  if 'pad' in ops:
    assert 'padding' in extra_params
  if 'local_contrast_normalization' in ops:
    assert 'lcn_filter_sigma' in extra_params
  if 'local_luminance_subtraction' in ops:
    assert 'lls_filter_sigma' in extra_params
  if 'standardize_data_range' in ops:
    idx_sdr = [i for i, op in enumerate(ops) if op == 'standardize_data_range']
    assert len(idx_sdr) == 1 and idx_sdr[0] == 0
  if isinstance(dataset, str):
    if dataset not in DATASETS:
      raise KeyError('Unrecognized dataset ' + dataset)
    if 'filepath' not in extra_params:
      raise KeyError('dataset %r: extra_params[\'filepath\'] is required '
                     '(there are no default data locations)' % dataset)
    if dataset == 'Kodak':
      raise NotImplementedError('This is next')
  flatten_patches = extra_params.get('flatten_patches', True)
  patched = False
  for op in ops:
    if op not in PREPROC_OPS:
      raise KeyError('Unrecognized preprocessing op ' + str(op))
    if op == 'patch':
      patched = True
    elif op in _BEFORE_PATCH and patched:
      raise KeyError(_BEFORE_PATCH[op])
    elif op in _AFTER_PATCH and not patched:
      raise KeyError(_AFTER_PATCH[op])
    elif op == 'pad' and flatten_patches:
      raise KeyError('Flattened patches shouldnt require padding')
  # the device filter's own condition: an odd (centred) Gaussian window
  if 'local_contrast_normalization' in ops:
    ip_util.gaussian_window(extra_params['lcn_filter_sigma'])
  if 'local_luminance_subtraction' in ops:
    ip_util.gaussian_window(extra_params['lls_filter_sigma'])


def _as_hwc(img):
  """One image as a float32 (h, w, c) array or tensor; 2D is (h, w, 1)."""
  if torch.is_tensor(img):
    img = img.to(torch.float32)
    return img[:, :, None] if img.dim() == 2 else img
  img = np.asarray(img).astype('float32')
  return img[:, :, None] if img.ndim == 2 else img


def _load_images(dataset, extra_params):
  """The reference's loaders (dataset_generation.py:121-153) and 'exclude'
  (:155-157); an image stack given directly is the extension.  Returns a
  list of float32 (h, w, c) numpy arrays or tensors."""
  if isinstance(dataset, str):
    filepath = extra_params['filepath']
    if dataset == 'Field_NW':
      import scipy.io
      raw = scipy.io.loadmat(filepath)['IMAGESr'].astype('float32')
      temp = np.transpose(raw, (2, 0, 1))
      images = [temp[x][:, :, None] for x in range(temp.shape[0])]
    elif dataset == 'vanHateren':
      try:
        import h5py
      except ImportError as e:
        raise ImportError('the vanHateren dataset is an HDF5 file: reading it '
                          'needs h5py, which is not installed') from e
      with h5py.File(filepath, 'r') as file_handle:
        temp = np.array(file_handle['van_hateren_good'], dtype='float32')
      images = [temp[x][:, :, None] for x in range(temp.shape[0])]
    else:  # 'Kodak_BW': a pickled list of uint8 arrays
      from training.sparse_coding import _ArrayUnpickler
      with open(filepath, 'rb') as f:
        raw = _ArrayUnpickler(f).load()
      if not isinstance(raw, (list, tuple)):
        raise pickle.UnpicklingError('Kodak_BW: expected a list of arrays')
      images = [np.asarray(x).astype('float32')[:, :, None] for x in raw]
  elif torch.is_tensor(dataset):
    assert dataset.dim() == 4, 'an image stack is (count, h, w, c)'
    images = [_as_hwc(x) for x in dataset]
  else:
    images = [_as_hwc(x) for x in dataset]
  if 'exclude' in extra_params:
    images = [images[x] for x in range(len(images))
              if x not in extra_params['exclude']]
  assert len(images) > 0, 'no images to draw patches from'
  return images


class _ImageGroups:
  """The images as device stacks of equal shape (whitening and the local
  filters run once per stack), with each image's (group, slot)."""

  def __init__(self, images, device):
    self.shapes = [tuple(int(v) for v in x.shape) for x in images]
    keys = sorted(set(self.shapes), key=self.shapes.index)
    self.group_of = np.array([keys.index(s) for s in self.shapes])
    self.slot_of = np.zeros(len(images), np.int64)
    self.stacks = []
    for g, key in enumerate(keys):
      members = np.nonzero(self.group_of == g)[0]
      self.slot_of[members] = np.arange(len(members))
      parts = [images[i] for i in members]
      if all(torch.is_tensor(x) for x in parts):
        stack = torch.stack([x.to(device) for x in parts])
      else:
        stack = torch.from_numpy(np.stack([
            x.cpu().numpy() if torch.is_tensor(x) else x for x in parts]))
      self.stacks.append(stack.to(device=device, dtype=torch.float32)
                         .contiguous())

  def map(self, fn):
    return [fn(s) for s in self.stacks]

  def gather(self, stacks, img_idx, vert, horz, patch_dimensions):
    """(num, ph, pw, c) patches of `stacks` (one per group) in the order of
    img_idx."""
    ph, pw = int(patch_dimensions[0]), int(patch_dimensions[1])
    if len(stacks) == 1:
      return extract_patches(stacks[0], img_idx, vert, horz,
                             patch_dimensions, flatten=False)
    c = stacks[0].shape[3]
    out = torch.empty((len(img_idx), ph, pw, c), dtype=torch.float32,
                      device=stacks[0].device)
    groups = self.group_of[img_idx]
    for g, stack in enumerate(stacks):
      sel = np.nonzero(groups == g)[0]
      if len(sel) == 0:
        continue
      out[torch.from_numpy(sel).to(out.device)] = extract_patches(
          stack, self.slot_of[img_idx[sel]], vert[sel], horz[sel],
          patch_dimensions, flatten=False)
    return out


def _standardize_groups(stacks):
  """standardize_data_range over all groups at once: one min and max."""
  if len(stacks) == 1:
    return [standardize_data_range(stacks[0])]
  flat = standardize_data_range(torch.cat([s.reshape(-1) for s in stacks]))
  sizes = [s.numel() for s in stacks]
  return [part.reshape(s.shape) for part, s in
          zip(torch.split(flat, sizes), stacks)]


def create_patch_training_set(num_samples, patch_dimensions, edge_buffer,
                              dataset, order_of_preproc_ops, extra_params={}):
  """
  The reference's create_patch_training_set (dataset_generation.py:22-311)
  with every preprocessing op on the device.

  dataset : 'Field_NW' (a .mat file holding IMAGESr (h, w, count)),
      'vanHateren' (HDF5, needs h5py) or 'Kodak_BW' (a pickled list of uint8
      (h, w) arrays, read without running any code the file names), located
      by extra_params['filepath'] -- there are no default locations -- or,
      as an extension, an image stack: a (count, h, w, c) tensor or a list of
      (h, w, c) arrays / tensors (images of different sizes allowed).
  order_of_preproc_ops, extra_params : as in the reference ('filepath',
      'exclude', 'padding', 'lcn_filter_sigma', 'lls_filter_sigma',
      'whitening_cutoff_low', 'whitening_cutoff_high', 'flatten_patches'),
      plus 'device' (default: the current HIP device).
  Every argument error of the reference is raised, with its exception type,
  before a file is read or the device is touched.  Patch positions come from
  numpy's global generator exactly as the reference draws them, which leaves
  the generator where the reference leaves it.

  Returns the reference's keys as float32 device tensors: 'patches' (d, n),
  or (d, c, ph, pw) with flatten_patches False; 'local_contrasts' /
  'local_luminances' (same layout) when LCN / LLS ran;
  'original_component_means' / 'original_component_variances' (n,);
  'ZCA_parameters' as whiten_ZCA returns them.
  """
  ops = list(order_of_preproc_ops)
  check_request(dataset, ops, extra_params)
  flatten_patches = extra_params.get('flatten_patches', True)
  wcl = extra_params.get('whitening_cutoff_low', 1e-3)
  wch = extra_params.get('whitening_cutoff_high', 0.9)
  images = _load_images(dataset, extra_params)
  device = extra_params.get('device')
  if device is None:
    device = (dataset.device if torch.is_tensor(dataset) and dataset.is_cuda
              else torch.device('cuda', torch.cuda.current_device()))
  groups = _ImageGroups(images, device)
  stacks = groups.stacks
  contrasts = luminances = None
  patches = patches_contrast = patches_luminance = None
  orig_means = orig_variances = zca_params = None

  def flat(a):
    return a.reshape(a.shape[0], -1)

  for op in ops:
    if op == 'standardize_data_range':
      stacks = _standardize_groups(stacks)
    elif op == 'whiten_center_surround':
      stacks = [ip_util.whiten_center_surround(
          s, cutoffs={'low': wcl, 'high': wch}, norm_and_threshold=False)
          for s in stacks]
    elif op == 'local_contrast_normalization':
      res = [ip_util.local_contrast_normalization(
          s, extra_params['lcn_filter_sigma'], return_normalizer=True)
          for s in stacks]
      stacks, contrasts = [r[0] for r in res], [r[1] for r in res]
    elif op == 'local_luminance_subtraction':
      res = [ip_util.local_luminance_subtraction(
          s, extra_params['lls_filter_sigma'], return_subtractor=True)
          for s in stacks]
      stacks, luminances = [r[0] for r in res], [r[1] for r in res]
    elif op == 'patch':
      img_idx, vert, horz = draw_patch_positions(
          num_samples, [s[:2] for s in groups.shapes], patch_dimensions,
          edge_buffer, len(groups.shapes))
      patches = groups.gather(stacks, img_idx, vert, horz, patch_dimensions)
      if 'local_contrast_normalization' in ops:
        patches_contrast = groups.gather(contrasts, img_idx, vert, horz,
                                         patch_dimensions)
      if 'local_luminance_subtraction' in ops:
        patches_luminance = groups.gather(luminances, img_idx, vert, horz,
                                          patch_dimensions)
    elif op == 'whiten_ZCA':
      white, zca_params = ip_util.whiten_ZCA(flat(patches))
      patches = white.reshape(patches.shape)
    elif op == 'center_each_component':
      temp, orig_means = ip_util.center_each_component(flat(patches))
      patches = temp.reshape(patches.shape)
    elif op == 'normalize_component_variance':
      temp, orig_variances = ip_util.normalize_component_variance(
          flat(patches))
      patches = temp.reshape(patches.shape)
    elif op == 'center_each_patch':
      temp, _ = ip_util.center_each_sample(flat(patches))
      patches = temp.reshape(patches.shape)
    elif op == 'pad':
      (top, bottom), (left, right) = extra_params['padding']
      amounts = (0, 0, int(left), int(right), int(top), int(bottom))

      def pad(a):
        return None if a is None else torch.nn.functional.pad(a, amounts)
      patches = pad(patches)
      patches_contrast = pad(patches_contrast)
      patches_luminance = pad(patches_luminance)

  def layout(a):
    if flatten_patches:
      return a.reshape(num_samples, -1)
    return a.permute(0, 3, 1, 2).contiguous()

  return_dict = {'patches': layout(patches)}
  if 'local_contrast_normalization' in ops:
    return_dict['local_contrasts'] = layout(patches_contrast)
  if 'local_luminance_subtraction' in ops:
    return_dict['local_luminances'] = layout(patches_luminance)
  if 'center_each_component' in ops:
    return_dict['original_component_means'] = orig_means
  if 'normalize_component_variance' in ops:
    return_dict['original_component_variances'] = orig_variances
  if 'whiten_ZCA' in ops:
    return_dict['ZCA_parameters'] = zca_params
  return return_dict
