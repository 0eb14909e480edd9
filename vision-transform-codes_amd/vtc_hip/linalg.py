"""
Covariance, symmetric eigen-decomposition and the ZCA row transform on the
device (csrc/zca.hip): the primitives behind utils.image_processing.whiten_ZCA
/ unwhiten_ZCA and training.pca.train_dictionary; the matrix inverse
(csrc/inverse.hip) behind analysis_transforms.fully_connected.
invertible_linear and training.ica.

Library routines stand in for a kernel of this engine in three documented
places only.  In symmetric_eigh: matrices larger than 256 x 256 (beyond the
single-workgroup Jacobi solver) and a Jacobi run that reports it did not
converge within JACOBI_MAX_SWEEPS sweeps (with a warning); both take
torch.linalg.eigh in float64 on the device.  In mat_inverse / inverse:
matrices larger than 256 x 256 take torch.linalg.inv_ex in float64 on the
device.
"""
import ctypes
import warnings

import torch

from . import (check, current_stream, load_library, ptr, require_device_tensor,
               workspace)

EIG_MAX_N = 256
# bound of the Jacobi iteration (quadratic convergence: 6-10 sweeps at n = 256)
JACOBI_MAX_SWEEPS = 30


def column_covariance(x, center, want_covariance=True):
  """x (D, n) float32 device tensor.  Returns (cov, means, grand_mean):
  cov (n, n) float64 = Xc^T Xc / D (None unless want_covariance), Xc = x -
  means when center else x; means (n,) float64 column means; grand_mean (1,)
  float64, the mean of the means."""
  lib = load_library()
  x = require_device_tensor(x, 'x').contiguous()
  rows, cols = x.shape
  dev = x.device
  means = torch.empty(cols, dtype=torch.float64, device=dev)
  grand = torch.empty(1, dtype=torch.float64, device=dev)
  cov = (torch.empty((cols, cols), dtype=torch.float64, device=dev)
         if want_covariance else None)
  ws = workspace(lib.vtc_column_covariance_workspace_bytes(rows, cols), dev)
  check(lib.vtc_column_covariance(
      ptr(x), rows, cols, 1 if center else 0, ptr(means), ptr(grand), ptr(cov),
      ptr(ws), ws.numel(), current_stream(dev)), 'vtc_column_covariance')
  return cov, means, grand


def sym_eig(a, max_sweeps=None):
  """Jacobi eigen-decomposition of a symmetric (n, n) float64 device matrix,
  n <= 256 (vtc_sym_eig).  Returns (eigvals (n,) float64 descending,
  eigvecs (n, n) float32 with the vectors as columns, status (2,) int32 device
  tensor [converged, sweeps]).  No host synchronisation."""
  lib = load_library()
  a = require_device_tensor(a, 'a', torch.float64).contiguous()
  n = a.shape[0]
  dev = a.device
  w = torch.empty(n, dtype=torch.float64, device=dev)
  u = torch.empty((n, n), dtype=torch.float32, device=dev)
  status = torch.zeros(2, dtype=torch.int32, device=dev)
  ws = workspace(lib.vtc_sym_eig_workspace_bytes(n), dev)
  sweeps = JACOBI_MAX_SWEEPS if max_sweeps is None else int(max_sweeps)
  check(lib.vtc_sym_eig(ptr(a), n, sweeps, ptr(w), ptr(u), ptr(status),
                        ptr(ws), ws.numel(), current_stream(dev)),
        'vtc_sym_eig')
  return w, u, status


def _signed_columns(u):
  """The sign rule of vtc_sym_eig applied to library eigenvectors: each
  column's largest-magnitude entry positive, ties to the lower index."""
  at = torch.argmax(u.abs(), dim=0)   # first maximum
  lead = u.gather(0, at[None, :])[0]
  return u * torch.where(lead < 0, -1.0, 1.0).to(u.dtype)[None, :]


def _library_eigh(a):
  w, u = torch.linalg.eigh(a.to(torch.float64))
  w, u = w.flip(0), u.flip(1)
  return w, _signed_columns(u.to(torch.float32))


def symmetric_eigh(a, max_sweeps=None):
  """(eigvals float64 descending, eigvecs float32 columns) of a symmetric
  float64 device matrix.  n <= 256: vtc_sym_eig, then one host read of its
  convergence flag; converged == 0 warns and falls back to
  torch.linalg.eigh.  n > 256: torch.linalg.eigh (float64, on the device).
  Both routes return the same descending order and sign rule."""
  n = a.shape[0]
  if n > EIG_MAX_N:
    return _library_eigh(a)
  w, u, status = sym_eig(a, max_sweeps)
  converged, sweeps = [int(v) for v in status.tolist()]
  if converged != 1:
    warnings.warn('vtc_sym_eig did not converge in %d Jacobi sweeps (n = %d); '
                  'falling back to torch.linalg.eigh' % (sweeps, n),
                  RuntimeWarning)
    return _library_eigh(a)
  return w, u


def zca_matrices(eigvecs, eigvals, eps=1e-4, whiten=True, unwhiten=True):
  """W = U diag(1/(sqrt(w)+eps)) U^T and W^-1 = U diag(sqrt(w)+eps) U^T,
  float64 sums rounded to float32 (vtc_zca_matrices).  eigvecs (n, n) float32
  columns, eigvals (n,) float64, both device tensors.  Returns (W, W_inv),
  None for the one not asked for."""
  lib = load_library()
  u = require_device_tensor(eigvecs, 'eigvecs').contiguous()
  w = require_device_tensor(eigvals, 'eigvals', torch.float64).contiguous()
  n = u.shape[0]
  w_mat = torch.empty((n, n), dtype=torch.float32, device=u.device) \
      if whiten else None
  w_inv = torch.empty((n, n), dtype=torch.float32, device=u.device) \
      if unwhiten else None
  check(lib.vtc_zca_matrices(ptr(u), ptr(w), n, ctypes.c_double(eps),
                             ptr(w_mat), ptr(w_inv),
                             current_stream(u.device)), 'vtc_zca_matrices')
  return w_mat, w_inv


def row_transform(x, offsets, matrix, add):
  """y = (x - offsets) matrix + add (vtc_row_transform); x (D, n), offsets
  (n,), matrix (n, n) float32 device tensors, add a Python float (used as
  float32)."""
  lib = load_library()
  x = require_device_tensor(x, 'x').contiguous()
  offsets = require_device_tensor(offsets, 'offsets').contiguous()
  matrix = require_device_tensor(matrix, 'matrix').contiguous()
  rows, n = x.shape
  y = torch.empty_like(x)
  check(lib.vtc_row_transform(ptr(x), rows, n, ptr(offsets), ptr(matrix),
                              float(add), ptr(y), current_stream(x.device)),
        'vtc_row_transform')
  return y


INVERSE_MAX_N = 256


def mat_inverse(a, status=None):
  """Inverse of an (n, n) float32 device matrix without a host
  synchronisation.  Returns (a_inv (n, n) float32, status (2,) int32 device
  tensor [nonsingular (1 / 0), first bad pivot index or -1]); `status` may be
  given as a (2,) int32 device tensor to write into.

  n <= 256: vtc_mat_inverse (float64 LU with partial pivoting, rounded once).
  n > 256: torch.linalg.inv_ex in float64 on the device, rounded to float32;
  the status then comes from its LU (and a finiteness check of the input)."""
  a = require_device_tensor(a, 'a').contiguous()
  if a.dim() != 2 or a.shape[0] != a.shape[1]:
    raise ValueError('a must be a square matrix, got shape %s'
                     % (tuple(a.shape),))
  n = a.shape[0]
  dev = a.device
  if status is None:
    status = torch.empty(2, dtype=torch.int32, device=dev)
  else:
    status = require_device_tensor(status, 'status', torch.int32)
    assert status.shape == (2,) and status.is_contiguous()
  if n > INVERSE_MAX_N:
    a_inv, info = torch.linalg.inv_ex(a.to(torch.float64))
    good = (info == 0) & torch.isfinite(a).all()
    status[0] = good.to(torch.int32)
    status[1] = torch.where(info > 0, info - 1, -1).to(torch.int32)
    return a_inv.to(torch.float32), status
  lib = load_library()
  a_inv = torch.empty_like(a)
  ws = workspace(lib.vtc_mat_inverse_workspace_bytes(n), dev)
  check(lib.vtc_mat_inverse(ptr(a), n, ptr(a_inv), ptr(status), ptr(ws),
                            ws.numel(), current_stream(dev)),
        'vtc_mat_inverse')
  return a_inv, status


def raise_if_singular(status, what='matrix'):
  """One host read of a mat_inverse status; raises torch.linalg.LinAlgError
  (what torch.inverse raises) for a singular or non-finite input."""
  nonsingular, bad = [int(v) for v in status.tolist()]
  if nonsingular != 1:
    if bad >= 0:
      raise torch.linalg.LinAlgError(
          'inverse: the %s is singular (pivot %d is zero or not finite)'
          % (what, bad))
    raise torch.linalg.LinAlgError(
        'inverse: the %s holds a non-finite value' % what)


def inverse(a, check=True):
  """a^-1 of an (n, n) float32 device matrix as float32 (mat_inverse).  With
  check=True one host read of the status raises torch.linalg.LinAlgError for
  a singular or non-finite input, as torch.inverse would."""
  a_inv, status = mat_inverse(a)
  if check:
    raise_if_singular(status)
  return a_inv
