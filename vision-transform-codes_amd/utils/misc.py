"""
The numeric part of the reference's utils/misc.py on device tensors:
rotational_average (misc.py:24-76) through vtc_binned_mean
(csrc/code_stats.hip behind include/vtc_stats.h), and
load_newest_dictionary_checkpoint under the reference's import path.
walk_on_unit_sphere is not provided.
"""
import numpy as np
import torch

import vtc_hip
from training.sparse_coding import load_newest_dictionary_checkpoint  # noqa

_bin_maps = {}      # (h, w, nbins) -> (bin_of int32 ndarray, left edges)
_device_maps = {}   # (h, w, nbins, device) -> bin_of on that device


def rotational_bin_map(shape, nbins, elem_cartesian_coords=None):
  """
  The radial bin of every element of an (h, w) array, on the host.

  Each element has a vertical and a horizontal coordinate, its own indices
  unless elem_cartesian_coords = (vertical, horizontal) gives them.  Its
  radius sqrt(horizontal^2 + vertical^2) is sorted into nbins equal bins
  between 0 and the largest coordinate magnitude of either axis; a radius
  equal to that largest magnitude belongs to the last bin, a larger one (the
  corners) to none.
  Returns (bin_of, left_edges): int32 (h, w) with nbins for "no bin", and the
  float64 left edge of every bin, both read-only (they are cached).
  """
  nbins = int(nbins)
  if nbins < 1:
    raise ValueError('nbins must be at least 1')
  h, w = (int(v) for v in shape)
  key = (h, w, nbins)
  if elem_cartesian_coords is None:
    if key in _bin_maps:
      return _bin_maps[key]
    vertical, horizontal = np.indices((h, w))
  else:
    vertical, horizontal = (np.asarray(v) for v in elem_cartesian_coords)
    if vertical.shape != (h, w) or horizontal.shape != (h, w):
      raise ValueError('coordinates of shape %s and %s for an array of %s'
                       % (vertical.shape, horizontal.shape, (h, w)))
  radius = np.sqrt(horizontal**2 + vertical**2)
  outermost = max(np.abs(horizontal).max(), np.abs(vertical).max())
  edges = np.linspace(0.0, outermost, nbins + 1)
  bin_of = np.searchsorted(edges, radius, side='right') - 1
  bin_of[radius == outermost] = nbins - 1   # the corners stay at nbins
  result = (np.ascontiguousarray(bin_of, dtype=np.int32), edges[:-1].copy())
  for array in result:   # the cached arrays are shared by every caller
    array.setflags(write=False)
  if elem_cartesian_coords is None:
    _bin_maps[key] = result
  return result


def binned_mean(images, bin_of, nbins):
  """
  The mean of every bin of a map, for a (count, h, w) float32 or float64
  device stack: vtc_binned_mean.  bin_of: int32 (h, w) device tensor, a value
  outside [0, nbins) belongs to no bin.  Returns (means, members): float64
  (count, nbins), NaN for an empty bin, and int64 (nbins,).  Only enqueues.
  """
  lib = vtc_hip.load_library()
  if not torch.is_tensor(images):
    raise TypeError('images must be a torch.Tensor')
  if images.dim() != 3 or min(images.shape) < 1:
    raise ValueError('images must be (count, h, w), got shape %s'
                     % (tuple(images.shape),))
  if images.dtype == torch.float64:
    x, code = vtc_hip.require_device_tensor(
        images, 'images', torch.float64).contiguous(), vtc_hip.DTYPE_F64
  else:
    x, code = (vtc_hip.require_device_tensor(images, 'images').contiguous(),
               vtc_hip.DTYPE_F32)
  count, h, w = x.shape
  m = vtc_hip.require_device_tensor(bin_of, 'bin_of', torch.int32).contiguous()
  if tuple(m.shape) != (h, w):
    raise ValueError('bin_of of shape %s for images of %s'
                     % (tuple(m.shape), (h, w)))
  nbins = int(nbins)
  device = x.device
  means = torch.empty((count, nbins), dtype=torch.float64, device=device)
  members = torch.empty(nbins, dtype=torch.int64, device=device)
  ws = vtc_hip.workspace(
      lib.vtc_binned_mean_workspace_bytes(count, h, w, nbins), device)
  vtc_hip.check(lib.vtc_binned_mean(
      vtc_hip.ptr(x), code, vtc_hip.ptr(m), count, h, w, nbins,
      vtc_hip.ptr(means), vtc_hip.ptr(members), vtc_hip.ptr(ws), ws.numel(),
      vtc_hip.current_stream(device)), 'vtc_binned_mean')
  return means, members


def rotational_average(array_2d, nbins=10, elem_cartesian_coords=None):
  """
  The mean of a 2-d array over rings of equal width around the origin of its
  coordinates (see rotational_bin_map), e.g. of a power spectrum.

  array_2d : (h, w) float32 or float64 device tensor, or a (count, h, w)
      stack of them.
  nbins : number of rings, at most 4096.
  elem_cartesian_coords : optional (vertical, horizontal) numpy arrays of
      shape (h, w); by default the element indices.
  Returns (rotational_means, magnitude_bins): a float64 device tensor (nbins,)
  -- (count, nbins) for a stack -- with NaN for a ring that holds no element,
  and the float64 numpy array of the rings' left edges.  The ring of every
  element is geometry: it is computed on the host once per (shape, nbins) and
  kept on the device.  Only enqueues.
  """
  if not torch.is_tensor(array_2d):
    raise TypeError('array_2d must be a torch.Tensor')
  if array_2d.dim() not in (2, 3):
    raise ValueError('array_2d must be (h, w) or (count, h, w), got shape %s'
                     % (tuple(array_2d.shape),))
  stack = array_2d if array_2d.dim() == 3 else array_2d[None]
  if not stack.is_cuda:
    raise vtc_hip.VtcHipError(
        'array_2d lives on %s: the MI355X engine only runs on HIP device '
        'tensors (no CPU path is provided on purpose)' % (stack.device,))
  h, w = stack.shape[1:]
  bin_of, edges = rotational_bin_map((h, w), nbins, elem_cartesian_coords)
  if elem_cartesian_coords is None:
    key = (h, w, int(nbins), str(stack.device))
    if key not in _device_maps:
      _device_maps[key] = torch.from_numpy(bin_of.copy()).to(stack.device)
    on_device = _device_maps[key]
  else:
    on_device = torch.from_numpy(bin_of.copy()).to(stack.device)
  means, _ = binned_mean(stack, on_device, nbins)
  return (means if array_2d.dim() == 3 else means[0]), edges.copy()
