"""The plugin layer inside `with torch.cuda.stream(s):`, behind a delay.

Every plugin hands vtc_hip.current_stream(device) to the C library and takes
its scratch from vtc_hip.workspace, its group tables from the cache of
vtc_hip/groups.py and, on the device step-size path, a pinned spectrum mirror.
The rest of the suite calls them with the default stream current.  Here one
smallest-shape call per plugin module runs twice:

  default   inputs uploaded and the plugin called on the default stream
  held      on a PyTorch pool stream `s` (tests/held_stream.py): the delay,
            then the upload of every input from pinned memory into tensors
            that hold 0xFF (NaN) until then, then the plugin, all with `s`
            current

and every result (returned tensors, tensors updated in place, host values)
must be torch.equal / equal to the default call's.  A library or plugin
operation that lands on another stream runs while `s` still sleeps and sees
the poison.  A canary taken on the null stream immediately before the plugin
call must still hold 0xFF, or the case proved nothing.  A second one, taken
when the plugin returns, tells whether the call only enqueued or blocked on a
host read; that is printed, not asserted (a plugin that returns a Python
number has to wait).  Step sizes are passed explicitly or taken on the device
path, so no inference case needs a host read before its work is enqueued.

The raw C ABI on a held stream is tests/test_stream_order_gpu.py.
"""
import numpy as np
import pytest
import torch

import held_stream
import helpers
import sc_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hold(device):
  return held_stream.hold(device)


def _flat(out):
  """The comparable leaves of a plugin's result, in a fixed order."""
  if out is None:
    return []
  if torch.is_tensor(out):
    return [out]
  if isinstance(out, dict):
    return [leaf for k in sorted(out) for leaf in _flat(out[k])]
  if isinstance(out, (tuple, list)) and any(
      torch.is_tensor(v) or isinstance(v, (dict, tuple, list)) for v in out):
    return [leaf for v in out for leaf in _flat(v)]
  return [out]


def run_both(device, hold, name, inputs, fn):
  """fn(tensors) -> result, where `tensors` maps each name of `inputs` to a
  device tensor; a tensor the plugin updates in place is part of what fn
  returns."""
  inputs = {k: torch.from_numpy(np.ascontiguousarray(v))
            for k, v in inputs.items()}
  want = _flat(fn({k: v.to(device) for k, v in inputs.items()}))
  torch.cuda.synchronize(device)
  assert want, name

  s = hold.streams[0]
  staged = {k: held_stream.poisoned_like(v, device) for k, v in inputs.items()}
  first = next(iter(staged.values()))[0]
  torch.cuda.synchronize(device)
  with torch.cuda.stream(s):
    hold.sleep()
    for t, host in staged.values():
      t.copy_(host, non_blocking=True)
    before = held_stream.canary(first)
    assert torch.cuda.current_stream(device) == s
    got, host_ms = held_stream.timed(
        lambda: _flat(fn({k: v[0] for k, v in staged.items()})))
    after = held_stream.canary(first)
  s.synchronize()
  torch.cuda.synchronize(device)
  assert held_stream.is_poison(before), (
      '%s proved nothing: the null stream saw the staged input before the '
      'plugin was called (delay %.1f ms)' % (name, hold.delay_ms))
  enqueued_only = held_stream.is_poison(after)

  assert len(got) == len(want), name
  for index, (g, w) in enumerate(zip(got, want)):
    if torch.is_tensor(w):
      assert g.shape == w.shape and g.dtype == w.dtype, (name, index)
      if w.dtype.is_floating_point:
        assert bool(torch.isfinite(g).all()), (
            '%s: result %d holds non-finite values on the side stream'
            % (name, index))
      assert torch.equal(g, w), (
          '%s: result %d differs from the default-stream call in %d of %d '
          'elements' % (name, index, int((g != w).sum()), w.numel()))
    else:
      assert g == w, (name, index, g, w)
  print('stream_order_plugin %-44s delay_ms %.1f call_ms %.3f canary ok, %s'
        % (name, hold.delay_ms, host_ms,
           'the call only enqueued' if enqueued_only else
           'the call blocked on a host read'))
  return enqueued_only


def _sparse(seed, shape, density=0.1, scale=0.05):
  rs = np.random.RandomState(seed)
  return (scale * rs.randn(*shape) * (rs.rand(*shape) < density)).astype(
      np.float32)


def _groups(count, m):
  return [list(range(g * m, g * m + m)) for g in range(count)]


def _conv_fixture():
  g = helpers.load('trainer')
  pad = tuple(tuple(int(v) for v in row) for row in g['conv_padding'])
  return (g['conv_images_padded'][:2].copy(), g['conv_dictionary0'].copy(),
          (4, 4), pad)


# ---------------------------------------------------------------- inference
def test_fc_fused_route(device, hold):
  """n = 256, s = 256, b = 64, f16x3, 10 iterations, the step size on the
  device path (vtc_gram, vtc_lambda_max_mirrored with the pinned mirror)."""
  from analysis_transforms.fully_connected import ista_fista
  assert ista_fista.fused_available()
  inputs = {'X': helpers.gaussian_patches(11, 64, 256),
            'D': helpers.unit_rows(12, 256, 256)}
  only = run_both(device, hold, 'fc ista_fista fused f16x3', inputs,
                  lambda t: ista_fista.run(t['X'], t['D'], 0.02, 10,
                                           precision='f16x3'))
  assert only, 'the device step-size path must not read the host'


def test_fc_tiled_route(device, hold):
  """n = 100, s = 96, b = 33, f32, an explicit step size."""
  from analysis_transforms.fully_connected import ista_fista
  D = helpers.unit_rows(14, 96, 100)
  eta = float(np.float32(sc_oracle.fc_stepsize(torch.from_numpy(D).double())))
  inputs = {'X': helpers.gaussian_patches(13, 33, 100), 'D': D}
  only = run_both(device, hold, 'fc ista_fista tiled f32', inputs,
                  lambda t: ista_fista.run(t['X'], t['D'], 0.02, 10,
                                           precision='f32', stepsize=eta))
  assert only, 'an explicit step size leaves nothing to read back'


def test_subspace(device, hold):
  """8 groups of 4, n = 64, b = 40: the group-table cache on a side stream."""
  from analysis_transforms.fully_connected import subspace_ista_fista
  groups = _groups(8, 4)
  inputs = {'X': helpers.gaussian_patches(15, 40, 64),
            'D': helpers.unit_rows(16, 32, 64)}
  run_both(device, hold, 'subspace_ista_fista', inputs,
           lambda t: subspace_ista_fista.run(t['X'], t['D'], groups, 0.03,
                                             10))


def test_conv(device, hold):
  """The trainer.npz geometry: 8 x 8 kernels, stride 4, 8 iterations."""
  from analysis_transforms.convolutional import ista_fista as conv
  imgs, K, stride, pad = _conv_fixture()
  eta = float(np.float32(sc_oracle.conv_stepsize(
      torch.from_numpy(K).double())))
  run_both(device, hold, 'conv ista_fista stride 4', {'X': imgs, 'K': K},
           lambda t: conv.run(t['X'], t['K'], stride, pad, 0.05, 8,
                              stepsize=eta))


def test_invertible_linear(device, hold):
  from analysis_transforms.fully_connected import invertible_linear
  rs = np.random.RandomState(17)
  q, _ = np.linalg.qr(rs.randn(16, 16))
  inputs = {'x': rs.randn(40, 16).astype(np.float32),
            'm': (q * (1.0 + rs.rand(16))[None, :]).astype(np.float32)}
  run_both(device, hold, 'invertible_linear n=16', inputs,
           lambda t: invertible_linear.run(t['x'], t['m']))


# ------------------------------------------------------------------ updates
def test_fc_dictionary_update(device, hold):
  from dict_update_rules.fully_connected import sc_steepest_descent
  inputs = {'X': helpers.gaussian_patches(18, 33, 100),
            'D': helpers.unit_rows(19, 96, 100), 'C': _sparse(20, (33, 96))}

  def step(t):
    sc_steepest_descent.run(t['X'], t['D'], t['C'], stepsize=0.1)
    return t['D']
  run_both(device, hold, 'fc sc_steepest_descent', inputs, step)


def test_subspace_dictionary_update(device, hold):
  from dict_update_rules.fully_connected import (
      subspace_sc_cheap_quadratic_descent as rule)
  groups = _groups(8, 4)
  inputs = {'X': helpers.gaussian_patches(21, 40, 64),
            'D': helpers.unit_rows(22, 32, 64), 'C': _sparse(23, (40, 32)),
            'H': (0.01 + np.random.RandomState(24).rand(32)).astype(
                np.float32)}

  def step(t):
    rule.run(t['X'], t['D'], t['C'], groups, t['H'], 0.1, stepsize=0.05)
    return t['D']
  run_both(device, hold, 'subspace_sc_cheap_quadratic_descent', inputs, step)


def test_conv_dictionary_update(device, hold):
  from dict_update_rules.convolutional import sc_steepest_descent
  imgs, K, stride, pad = _conv_fixture()
  side = (imgs.shape[2] - 8) // 4 + 1
  inputs = {'X': imgs, 'K': K,
            'C': _sparse(25, (imgs.shape[0], K.shape[0], side, side), 0.2)}

  def step(t):
    sc_steepest_descent.run(t['X'], t['K'], t['C'], stride, pad,
                            stepsize=0.005)
    return t['K']
  run_both(device, hold, 'conv sc_steepest_descent', inputs, step)


def test_ica_natural_gradient(device, hold):
  from dict_update_rules.fully_connected import ica_natural_gradient
  rs = np.random.RandomState(26)
  q, _ = np.linalg.qr(rs.randn(16, 16))
  inputs = {'D': q.astype(np.float32),
            'C': rs.laplace(size=(40, 16)).astype(np.float32)}

  def step(t):
    ica_natural_gradient.run(t['D'], t['C'], stepsize=0.01)
    return t['D']
  run_both(device, hold, 'ica_natural_gradient n=16', inputs, step)


# ------------------------------------------------------------- image tools
def _image(seed, h=37, w=53, c=3):
  return np.random.RandomState(seed).rand(h, w, c).astype(np.float32)


def test_zca(device, hold):
  """whiten_ZCA estimating on 200 x 16 (it reads the grand mean back: the
  call blocks), then unwhiten_ZCA with the parameters it returned."""
  from utils import image_processing as ip
  rs = np.random.RandomState(27)
  x = (rs.randn(200, 16) @ rs.randn(16, 16)).astype(np.float32)

  def both(t):
    white, params = ip.whiten_ZCA(t['x'])
    return white, params, ip.unwhiten_ZCA(white, params)
  run_both(device, hold, 'whiten_ZCA / unwhiten_ZCA 200x16', {'x': x}, both)


def test_whiten_center_surround(device, hold):
  from utils import image_processing as ip
  run_both(device, hold, 'whiten_center_surround 37x53x3',
           {'image': _image(28)},
           lambda t: ip.whiten_center_surround(t['image'],
                                               {'low': 0.1, 'high': 0.8}))


def test_filter_fd(device, hold):
  from utils import image_processing as ip
  rs = np.random.RandomState(29)
  filt = rs.randn(37, 53) + 1j * rs.randn(37, 53)
  run_both(device, hold, 'filter_fd 37x53x3',
           {'image': _image(30), 'filter': filt},
           lambda t: ip.filter_fd(t['image'], t['filter']))


def test_local_contrast_normalization(device, hold):
  from utils import image_processing as ip
  run_both(device, hold, 'local_contrast_normalization sigma 2',
           {'image': _image(31)},
           lambda t: ip.local_contrast_normalization(t['image'], 2.0))


def test_patches_and_assembly(device, hold):
  from utils import image_processing as ip

  def both(t):
    patches, positions = ip.patches_from_single_image(t['image'], (8, 8),
                                                      False)
    image = ip.assemble_image_from_patches(patches, (8, 8), positions)
    return patches, [tuple(p) for p in positions], image
  run_both(device, hold, 'patches_from_single_image / assemble',
           {'image': _image(32)}, both)


def test_compute_psnr(device, hold):
  """Returns a Python float: the call has to wait for its stream."""
  from utils import plotting
  target = _image(33)
  inputs = {'t': target,
            'r': target + 0.01 * np.random.RandomState(34).randn(
                *target.shape).astype(np.float32)}
  only = run_both(device, hold, 'compute_pSNR', inputs,
                  lambda t: plotting.compute_pSNR(t['t'], t['r']))
  assert not only
