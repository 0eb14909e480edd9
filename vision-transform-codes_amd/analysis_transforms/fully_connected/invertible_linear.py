"""
Codes through the exact inverse of a square dictionary on MI355X.

Drop-in for vision_transform_codes/analysis_transforms/fully_connected/
invertible_linear.py:6-28: same `run` signature and return value.  The filter
matrix is the float64-LU inverse of the dictionary rounded once to float32
(vtc_mat_inverse, vtc_hip.linalg.mat_inverse), or its transpose when
orthonormal=True; the codes are the float32 FMA chains of vtc_row_transform
with zero offsets.
"""
import torch

import vtc_hip
from vtc_hip import linalg


def _check_shapes(images, dictionary):
  if dictionary.dim() != 2 or dictionary.shape[0] != dictionary.shape[1]:
    raise ValueError('invertible_linear needs a square (n, n) dictionary, got '
                     'shape %s' % (tuple(dictionary.shape),))
  if images.dim() != 2 or images.shape[1] != dictionary.shape[0]:
    raise ValueError('images must be (b, %d), got shape %s'
                     % (dictionary.shape[0], tuple(images.shape)))


def apply_filter(images, filter_matrix):
  """codes (b, n) = images (b, n) @ filter_matrix (n, n), float32 FMA chains
  in k order on the device.  Only enqueues."""
  zeros = torch.zeros(filter_matrix.shape[0], dtype=torch.float32,
                      device=filter_matrix.device)
  return linalg.row_transform(images, zeros, filter_matrix, 0.0)


def run(images, dictionary, orthonormal=False):
  """
  Infers the code using the exact matrix inverse of the dictionary matrix.

  Parameters
  ----------
  images : torch.Tensor(float32, size=(b, n)) on a HIP device
  dictionary : torch.Tensor(float32, size=(n, n)) on a HIP device; never
      written
  orthonormal : bool, optional
      Take the transpose instead of the inverse.  Default False.

  Returns
  -------
  codes : torch.Tensor(float32, size=(b, n)), freshly allocated

  A singular or non-finite dictionary raises torch.linalg.LinAlgError, as the
  reference's torch.inverse does; that check reads the inverse's status back
  (one host synchronisation).  training.ica keeps the status on the device
  instead.
  """
  images = vtc_hip.require_device_tensor(images, 'images').contiguous()
  dictionary = vtc_hip.require_device_tensor(
      dictionary, 'dictionary').contiguous()
  _check_shapes(images, dictionary)
  if orthonormal:
    filter_matrix = dictionary.t().contiguous()
  else:
    filter_matrix = linalg.inverse(dictionary, check=True)
  return apply_filter(images, filter_matrix)
