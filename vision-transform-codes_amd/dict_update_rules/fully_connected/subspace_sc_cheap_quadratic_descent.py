"""
Hessian-diagonal-scaled dictionary update with a within-group alignment
penalty, for subspace sparse coding on MI355X.

Drop-in for vision_transform_codes/dict_update_rules/fully_connected/
subspace_sc_cheap_quadratic_descent.py:13-127.  The penalty gradient (sum over
the other members j of a group of sign(cos_ij) (d_j - cos_ij d_i), or its
norm-aware form for un-normalised dictionaries) is computed by one HIP block
per group instead of a Python loop over groups.  A group whose LDS tile does
not fit the kernel (alignment_fits_device) has its penalty gradient formed in
float64 torch instead, with a warning.
"""
import warnings

import torch

import vtc_hip
from vtc_hip import groups as group_tables
from dict_update_rules.fully_connected import _common


# limits of vtc_subspace_alignment_gradient (csrc/dict_update.hip): one thread
# per member, and a tile of (m n + m^2 + m) floats in 160 KiB of LDS
ALIGNMENT_MAX_GROUP = 256
ALIGNMENT_MAX_LDS = 160 * 1024


def alignment_fits_device(m, n):
  """Whether groups of m atoms of n pixels run on the HIP kernel."""
  return m <= ALIGNMENT_MAX_GROUP and (m * n + m * m + m) * 4 <= (
      ALIGNMENT_MAX_LDS)


def alignment_gradient_float64(dictionary, group_assignments,
                               dict_is_normalized):
  """The penalty gradient in float64 torch on the dictionary's device, summed
  over groups in group order (subspace_sc_cheap_quadratic_descent.py:91-127),
  rounded once to float32."""
  d = dictionary.double()
  total = torch.zeros_like(d)
  for members in group_assignments:
    idx = torch.tensor([int(a) for a in members], device=d.device)
    rows = d[idx]
    # grad_i = sum_j sign(cos_ij) (d_j / outer_ij - cos_ij d_i / |d_i|^2)
    if dict_is_normalized:
      cos = torch.mm(rows, rows.t())
      toward_other = torch.mm(torch.sign(cos), rows)
      toward_self = cos.abs().sum(1, keepdim=True) * rows
    else:
      norms = torch.norm(rows, p=2, dim=1, keepdim=True)
      outer = torch.mm(norms, norms.t())
      cos = torch.mm(rows, rows.t()) / outer
      toward_other = torch.mm(torch.sign(cos) / outer, rows)
      toward_self = cos.abs().sum(1, keepdim=True) * rows / norms ** 2
    total.index_add_(0, idx, toward_other - toward_self)
  return total.float()


def run(images, dictionary, codes, group_assignments, hessian_diagonal,
        alignment_penalty, stepsize=0.001, num_iters=1, lowest_code_val=0.001,
        normalize_dictionary=True):
  """
  images (b, n), dictionary (s, n) [updated IN PLACE], codes (b, s),
  hessian_diagonal (s,), group_assignments as in subspace_ista_fista.
  Returns None.
  """
  penalty = None
  if alignment_penalty != 0:
    lib = vtc_hip.load_library()
    vtc_hip.require_device_tensor(dictionary, 'dictionary')
    s, n = dictionary.shape
    device = dictionary.device
    tables = group_tables.tables_for(group_assignments, s, device)
    if not alignment_fits_device(tables.m, n):
      warnings.warn(
          'alignment penalty: groups of %d atoms x %d pixels exceed the LDS '
          'tile of vtc_subspace_alignment_gradient; computing its gradient in '
          'float64 torch' % (tables.m, n), RuntimeWarning)

      def compute_penalty_gradient():
        return alignment_gradient_float64(dictionary, group_assignments,
                                          normalize_dictionary)
    else:
      ws = vtc_hip.workspace(
          lib.vtc_subspace_alignment_gradient_workspace_bytes(tables.slots,
                                                              n), device)
      penalty_grad = torch.empty((s, n), dtype=torch.float32, device=device)

      def compute_penalty_gradient():
        vtc_hip.check(lib.vtc_subspace_alignment_gradient(
            vtc_hip.ptr(dictionary), vtc_hip.ptr(tables.index),
            vtc_hip.ptr(tables.valid), vtc_hip.ptr(tables.atom_ptr),
            vtc_hip.ptr(tables.atom_slots), vtc_hip.ptr(penalty_grad), s, n,
            tables.num_groups, tables.m, 1 if normalize_dictionary else 0,
            vtc_hip.ptr(ws), ws.numel(), vtc_hip.current_stream(device)),
            'vtc_subspace_alignment_gradient')
        return penalty_grad

    penalty = (float(alignment_penalty), compute_penalty_gradient)
  _common.descend(images, dictionary, codes, stepsize, num_iters,
                  normalize_dictionary, hessian_diagonal=hessian_diagonal,
                  lowest_code_val=lowest_code_val, penalty=penalty)
