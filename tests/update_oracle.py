"""Float64 restatement of the dictionary updates, split like the C ABI into a
gradient sum and an apply step, and the gates of tests/test_update_routes_gpu.py.

The gradient of a single update barely moves the dictionary, so a gate on the
updated dictionary D hides gradient errors.  The route tests gate the step
(D_after - D0) instead, at a step size that moves D by a few percent; the
host tests (tests/test_update_gates_host.py) show that every step gate catches
a 1e-4 relative error in the gradient.  Measured errors behind the gates:
profiles/precision_updates.txt.
"""
import numpy as np
import torch
import torch.nn.functional as F

import sc_oracle

LOWEST_CODE_VAL = 1e-3
STEP_FRACTION = 0.03       # ||D_after - D0|| / ||D0|| the tests aim for
MIN_STEP_FRACTION = 1e-2   # and assert after the per-row normalisation

# relative error of grad_sum against float64, per gradient route: the largest
# error measured on an MI355X over the route's cases, times at most 3
GRAD_GATES = {
    'fc-small': 3e-7,            # measured 1.15e-7
    'fc-split-k': 3e-7,          # 1.06e-7
    'conv-bf16x3': 1.2e-5,       # 4.50e-6
    'conv-patch-small': 4e-7,    # 1.60e-7
    'conv-patch': 3e-7,          # 1.20e-7
    'conv-unit': 8e-7,           # 3.02e-7
    'conv-direct': 4e-7,         # 1.62e-7
    'alignment': 5e-7,           # 1.87e-7
}
# relative error of the step D_after - D0 against the float64 step.  Its floor
# is the float32 rounding of D itself over a step of a few percent of D.
STEP_GATES = {
    'fc': 8e-6,                  # 3.01e-6
    'subspace': 5e-6,            # 1.87e-6
    'conv-f32': 7e-6,            # 2.62e-6
    'conv-bf16x3': 1.5e-5,       # 5.59e-6
}
ENERGY_GATE = 1.2e-7       # vtc_code_energy, vtc_hessian_ema: 4.60e-8
PERTURBATION = 1e-4        # gradient error every step gate must catch


def rel(a, b):
  a = torch.as_tensor(a).double()
  b = torch.as_tensor(b).double()
  return float((a - b).norm() / b.norm().clamp_min(1e-300))


def step_error(d_ours, d_ref, d0):
  """Relative error of the step (d_ours - d0) against (d_ref - d0)."""
  d0 = torch.as_tensor(d0).double()
  return rel(torch.as_tensor(d_ours).double() - d0,
             torch.as_tensor(d_ref).double() - d0)


def step_fraction(d_after, d0):
  d0 = torch.as_tensor(d0).double()
  return float((torch.as_tensor(d_after).double() - d0).norm() / d0.norm())


def perturb(grad, relative, seed=0):
  """grad + relative * ||grad|| * r / ||r||, r Gaussian (float64)."""
  grad = torch.as_tensor(grad).double()
  r = torch.from_numpy(np.random.RandomState(seed).randn(*grad.shape)).to(
      grad.device)
  return grad + relative * grad.norm() * r / r.norm()


# ------------------------------------------------------------ fully connected
def fc_gradient_sum(images, dictionary, codes):
  """C^T (C D - X), not divided by b (vtc_fc_dict_gradient)."""
  return sc_oracle.fc_gradient(images.double(), dictionary.double(),
                               codes.double()) * codes.shape[0]


def alignment_gradient_sum(dictionary, group_assignments, dict_is_normalized):
  """Sum over groups of sc_oracle.alignment_gradients, in float64."""
  d = dictionary.double()
  total = torch.zeros_like(d)
  for members in group_assignments:
    members = [int(a) for a in members]
    total[members] += sc_oracle.alignment_gradients(d[members],
                                                    dict_is_normalized)
  return total


def fc_apply(d0, grad_sum, batch, stepsize, hessian=None, penalty_grad=None,
             alignment_penalty=0.0, normalize=True):
  """vtc_fc_dict_apply in float64."""
  grad = grad_sum.double() / batch
  if penalty_grad is not None:
    grad = grad + alignment_penalty * penalty_grad.double()
  step = stepsize * grad
  if hessian is not None:
    step = step / (hessian.double()[:, None] + LOWEST_CODE_VAL)
  d = d0.double() - step
  if normalize:
    d = d / d.norm(dim=1, keepdim=True)
  return d


def fc_stepsize(d0, grad_sum, batch, hessian=None, penalty_grad=None,
                alignment_penalty=0.0):
  """The step size at which the un-normalised step is STEP_FRACTION of D."""
  unit = fc_apply(d0, grad_sum, batch, 1.0, hessian, penalty_grad,
                  alignment_penalty, normalize=False) - d0.double()
  return float(STEP_FRACTION * d0.double().norm() / unit.norm())


# ------------------------------------------------------------- convolutional
def conv_gradient_sum(images_padded, dictionary, codes, kernel_stride,
                      padding_dims):
  """sum over b of sc_oracle.conv_gradient, as im2col products in float64
  (runs on the device for the large cases; tests/test_update_gates_host.py
  pins it to sc_oracle.conv_gradient)."""
  x = images_padded.double()
  d = dictionary.double()
  c = codes.double()
  b, _, height, width = x.shape
  s, _, kh, kw = d.shape
  cols = torch.einsum('st,bsl->btl', d.reshape(s, -1), c.reshape(b, s, -1))
  recon = F.fold(cols, (height, width), (kh, kw), stride=kernel_stride)
  residual = sc_oracle.conv_mask(x, padding_dims) * (recon - x)
  patches = F.unfold(residual, (kh, kw), stride=kernel_stride)
  return torch.einsum('bsl,btl->st', c.reshape(b, s, -1),
                      patches).reshape(d.shape)


def conv_apply(d0, grad_sum, batch, stepsize, hessian=None, normalize=True):
  """vtc_conv_dict_apply in float64: optional Hessian divide, rescale to
  ||D||_F, step, per-kernel normalisation."""
  grad = grad_sum.double() / batch
  if hessian is not None:
    grad = grad / (hessian.double()[:, None, None, None] + LOWEST_CODE_VAL)
  d0 = d0.double()
  grad = grad * (d0.norm() / grad.norm())
  d = d0 - stepsize * grad
  if normalize:
    d = d / d.pow(2).sum(dim=(1, 2, 3), keepdim=True).sqrt()
  return d
