"""
The reference's training/pca.py (:8-39) on the device: the PCA dictionary in
one step, from the float64 covariance (csrc/zca.hip) and the Jacobi
eigen-decomposition of vtc_hip.linalg.
"""
import numpy as np
import torch

import vtc_hip
from vtc_hip import linalg


def train_dictionary(image_dataset):
  """
  image_dataset : (D, n) float32 device tensor, one sample per row; every
      column must be mean zero (|mean| < 1e-4, asserted as the reference does,
      with the means computed on the device).

  Returns the PCA dictionary U^T, (n, n) float32 on the device: row i is the
  i-th principal direction, in order of descending variance, signed so that
  its largest-magnitude component is positive (the reference's sign comes
  from its SVD and is arbitrary).

  n <= D and n <= 256: covariance X^T X / D in float64 and vtc_sym_eig.
  Fallbacks (torch.linalg in float64 on the device): n > D takes the SVD of
  the data as the reference does and returns (min(n, D), n) = (D, n);
  n > 256, or a Jacobi run that reports no convergence (with a warning),
  takes torch.linalg.eigh of the device covariance.
  """
  x = vtc_hip.require_device_tensor(image_dataset, 'image_dataset')
  x = x.contiguous()
  num_samples, n = x.shape
  if n > num_samples:
    _, means, _ = linalg.column_covariance(x, center=False,
                                           want_covariance=False)
    assert np.all(np.abs(means.cpu().numpy()) < 1e-4)
    u, _, _ = torch.linalg.svd(x.t().to(torch.float64), full_matrices=False)
    u = linalg._signed_columns(u.to(torch.float32))
    return u.t().contiguous()
  cov, means, _ = linalg.column_covariance(x, center=False)
  assert np.all(np.abs(means.cpu().numpy()) < 1e-4)
  _, u = linalg.symmetric_eigh(cov)
  return u.t().contiguous()
