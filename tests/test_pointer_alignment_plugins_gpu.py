"""The plugins on tensors whose data pointer is not 16-byte aligned.

`.contiguous()` keeps a view's storage offset, so `patches[1:]` of 7x7
patches, `images[1:]` of 70x93 images and a dictionary kept inside a larger
parameter buffer reach the C library 4 or 8 bytes off a 16-byte boundary.
Every case runs under the DEFAULT precision (or the one it names), must not
raise, and is held to the float64 oracle at the gate of the existing test of
that route (named at each case).  A tensor a call updates in place is updated
IN the view, and the buffer around it stays as it was.

Reference fixtures are used where one has the shape: fc_c2_mini.npz (64 x 256
patches, 1024 atoms, T = 20) for the fused kernel and conv.npz `k8s4_ragged`
for the stride-4 patch route.  The other shapes the cases need (b = 33,
s = 256 / 1280, 100 x 200, 7x7 patches, 70x93 images with 32 kernels of 11x11,
two channels of 5x5) have no fixture and use the float64 oracle.

The raw C ABI on such pointers is tests/test_pointer_alignment_gpu.py.
"""
import numpy as np
import pytest
import torch

import helpers
import sc_oracle

pytestmark = pytest.mark.gpu

CANARY = 1234.5
SPLIT_TOL, SPLIT_FLIP = helpers.REL_TOL_SHORT, helpers.NEAR_THRESHOLD


def skewed(t, elements=1):
  """A contiguous view holding `t`, `elements` elements into a buffer that is
  that much longer (the spare elements hold CANARY)."""
  buf = torch.full((t.numel() + elements,), CANARY, dtype=t.dtype,
                   device=t.device)
  view = buf[elements:].view(t.shape)
  view.copy_(t)
  assert view.is_contiguous() and view.data_ptr() % 16 != 0
  assert view.data_ptr() == buf.data_ptr() + elements * t.element_size()
  view.skew_buffer = buf
  return view


def _spare_untouched(view, elements=1):
  return bool((view.skew_buffer[:elements] == CANARY).all())


@pytest.fixture(scope='module')
def fc():
  from analysis_transforms.fully_connected import ista_fista
  if not ista_fista.fused_available():
    pytest.fail('libvtc_hip.so was built without the fused FISTA kernel')
  return ista_fista


_FC_REF = {}


def _fc_case(b, n, s, iters, warm):
  """(X, D, initial or None, eta, float64 oracle codes), computed once."""
  key = (b, n, s, iters, warm)
  if key not in _FC_REF:
    X = helpers.gaussian_patches(900 + b + s, b, n)
    D = helpers.unit_rows(901 + n + s, s, n)
    rs = np.random.RandomState(s + b)
    init = ((0.05 * rs.randn(b, s) * (rs.rand(b, s) < 0.1)).astype(np.float32)
            if warm else None)
    eta = float(np.float32(sc_oracle.fc_stepsize(
        torch.from_numpy(D).double())))
    ref = sc_oracle.fc_ista_fista(
        torch.from_numpy(X).double(), torch.from_numpy(D).double(), 0.02,
        iters, initial_codes=(torch.from_numpy(init).double() if warm
                              else None), stepsize=eta)
    _FC_REF[key] = (X, D, init, eta, ref.numpy())
  return _FC_REF[key]


def _run_fc(fc, device, case, which, precision=None, iters=20):
  X, D, init, eta, ref = case
  t = {'images': helpers.to_dev(X, device),
       'dictionary': helpers.to_dev(D, device),
       'initial_codes': (helpers.to_dev(init, device) if init is not None
                         else None)}
  t[which] = skewed(t[which])
  before = t[which].clone()
  out = fc.run(t['images'], t['dictionary'], 0.02, iters,
               initial_codes=t['initial_codes'], precision=precision,
               stepsize=eta)
  torch.cuda.synchronize(device)
  assert torch.equal(t[which], before) and _spare_untouched(t[which])
  return out.cpu().numpy(), ref


@pytest.mark.parametrize('which', ['images', 'dictionary', 'initial_codes'])
@pytest.mark.parametrize('s', [256, 1024])
def test_fc_fused_shapes(device, fc, s, which):
  """Gate: test_fc_fused_gpu.py::test_ragged_batch_sizes, f16x3."""
  import vtc_hip
  assert fc._resolve_precision(None, 33, 256, s, None) == vtc_hip.F16X3
  out, ref = _run_fc(fc, device, _fc_case(33, 256, s, 20, True), which)
  helpers.assert_codes_match(out, ref, SPLIT_TOL, 'fused s=%d, skewed %s'
                             % (s, which), max_flip_mag=SPLIT_FLIP)


@pytest.mark.parametrize('which', ['images', 'dictionary'])
def test_fc_fused_against_the_reference_fixture(device, fc, which):
  """fc_c2_mini.npz: the reference's own codes after 20 FISTA steps.  Gate:
  test_fc_fused_gpu.py::test_split_modes_match_reference_trace, f16x3."""
  g = helpers.load('fc_c2_mini')
  t = {'images': helpers.to_dev(helpers.gaussian_patches(0, 64, 256), device),
       'dictionary': helpers.to_dev(helpers.unit_rows(1, 1024, 256), device)}
  t[which] = skewed(t[which])
  out = fc.run(t['images'], t['dictionary'], float(g['sparsity_weight']), 20,
               stepsize=float(g['stepsize']))
  helpers.assert_codes_match(out.cpu().numpy(), g['codes_fista_T20'],
                             SPLIT_TOL, 'fc_c2_mini, skewed ' + which,
                             max_flip_mag=SPLIT_FLIP)
  assert _spare_untouched(t[which])


@pytest.mark.parametrize('which', ['images', 'dictionary', 'initial_codes'])
def test_fc_streamed_shape(device, fc, which):
  """Gate: test_fused_stream_gpu.py (5e-6, flips below 2e-6)."""
  out, ref = _run_fc(fc, device, _fc_case(33, 256, 1280, 20, True), which)
  helpers.assert_codes_match(out, ref, 5e-6, 'streamed, skewed %s' % which,
                             max_flip_mag=2e-6)


@pytest.mark.parametrize('precision', ['f16x3', 'auto'])
@pytest.mark.parametrize('b,n,s', [(130, 100, 200), (608, 400, 1000)])
def test_fc_tiled_split_route_on_a_dictionary_view(device, fc, b, n, s,
                                                   precision):
  """The tiled split route used to answer VTC_ERR_UNSUPPORTED for a
  dictionary that is not 16-byte aligned, and 'auto' picks f16x3 by shape
  alone above 2.4e8 multiply-adds (the second shape).  Gate: the fence
  table's for the tiled f16x3 route (REL_TOL_SHORT)."""
  import vtc_hip
  if (b, n, s) == (608, 400, 1000):
    assert b * n * s >= 240000000
    assert fc._resolve_precision('auto', b, n, s, None) == vtc_hip.F16X3
  out, ref = _run_fc(fc, device, _fc_case(b, n, s, 20, False), 'dictionary',
                     precision=precision)
  helpers.assert_codes_match(out, ref, SPLIT_TOL, 'tiled %s %dx%dx%d'
                             % (precision, b, n, s), max_flip_mag=SPLIT_FLIP)


def test_minibatch_slice_of_odd_patches(device, fc):
  """X[1:] of 7x7 patches starts 196 bytes into the storage."""
  b, n, s = 65, 49, 98
  X = helpers.gaussian_patches(77, b + 1, n)
  D = helpers.unit_rows(78, s, n)
  eta = float(np.float32(sc_oracle.fc_stepsize(torch.from_numpy(D).double())))
  ref = sc_oracle.fc_ista_fista(torch.from_numpy(X[1:]).double(),
                                torch.from_numpy(D).double(), 0.02, 20,
                                stepsize=eta)
  Xd = helpers.to_dev(X, device)
  view = Xd[1:]
  assert view.is_contiguous() and view.data_ptr() % 16 == 4
  out = fc.run(view, helpers.to_dev(D, device), 0.02, 20, stepsize=eta)
  helpers.assert_codes_match(out.cpu().numpy(), ref.numpy(),
                             helpers.REL_TOL_SHORT, 'X[1:], 7x7 patches')
  assert torch.equal(Xd.cpu(), torch.from_numpy(X))


@pytest.mark.parametrize('which', ['images', 'dictionary'])
@pytest.mark.parametrize('m', [4, 8])
def test_subspace_groups(device, m, which):
  """Gate: test_subspace_gpu.py::test_group_sizes_against_oracle, f32 and
  tight f16x3 (REL_TOL_SHORT)."""
  from analysis_transforms.fully_connected import subspace_ista_fista as sub
  num_groups, n = 20, 64
  s = num_groups * m
  groups = [list(range(g * m, g * m + m)) for g in range(num_groups)]
  X = helpers.gaussian_patches(500 + m, 40, n)
  D = helpers.unit_rows(501 + m, s, n)
  ref = sc_oracle.subspace_ista_fista(torch.from_numpy(X).double(),
                                      torch.from_numpy(D).double(), groups,
                                      0.03, 25)
  t = {'images': helpers.to_dev(X, device),
       'dictionary': helpers.to_dev(D, device)}
  t[which] = skewed(t[which])
  for precision in (None, 'f16x3'):
    out = sub.run(t['images'], t['dictionary'], groups, 0.03, 25,
                  precision=precision)
    helpers.assert_codes_match(out.cpu().numpy(), ref.numpy(),
                               helpers.REL_TOL_SHORT,
                               'groups of %d, skewed %s, %s'
                               % (m, which, precision))
  assert _spare_untouched(t[which])


def _ragged_groups(count, m):
  """Groups of 1..m atoms, the first of m; every third one shares an atom
  with the group before it (overlap); two atoms of the dictionary belong to
  no group.  Returns (groups, atoms)."""
  out, a = [], 0
  for g in range(count):
    size = 1 + (g * 5 + 2) % m if g else m
    members = list(range(a, a + size))
    a += size
    if g % 3 == 2:
      members[0] = out[-1][0]
    out.append(members)
  return out, a + 2


@pytest.mark.parametrize('which', ['images', 'dictionary'])
@pytest.mark.parametrize('m', [4, 8])
def test_subspace_ragged_groups(device, m, which):
  """Ragged, overlapping groups whose largest has m atoms: the padded
  index / valid tables, the gather of a skewed dictionary into padded slots
  and the scatter-add of shared atoms.  Gate: REL_TOL_SHORT
  (test_subspace_gpu.py::test_ragged_overlapping_groups)."""
  from analysis_transforms.fully_connected import subspace_ista_fista as sub
  groups, s = _ragged_groups(20, m)
  assert max(len(g) for g in groups) == m
  assert min(len(g) for g in groups) < m
  n = 64
  X = helpers.gaussian_patches(520 + m, 40, n)
  D = helpers.unit_rows(521 + m, s, n)
  ref = sc_oracle.subspace_ista_fista(torch.from_numpy(X).double(),
                                      torch.from_numpy(D).double(), groups,
                                      0.03, 25)
  t = {'images': helpers.to_dev(X, device),
       'dictionary': helpers.to_dev(D, device)}
  t[which] = skewed(t[which])
  before = t[which].clone()
  for precision in (None, 'f16x3'):
    out = sub.run(t['images'], t['dictionary'], groups, 0.03, 25,
                  precision=precision)
    helpers.assert_codes_match(out.cpu().numpy(), ref.numpy(),
                               helpers.REL_TOL_SHORT,
                               'ragged groups up to %d, skewed %s, %s'
                               % (m, which, precision))
  assert torch.equal(t[which], before) and _spare_untouched(t[which])


def _conv_case(seed, k, s, height, width, b, c=1, frame=None):
  rs = np.random.RandomState(seed)
  pad = k - 1 if frame is None else frame
  imgs = np.zeros((b, c, height + 2 * pad, width + 2 * pad), np.float32)
  imgs[:, :, pad:pad + height, pad:pad + width] = (
      0.5 * rs.randn(b, c, height, width)).astype(np.float32)
  D = rs.randn(s, c, k, k).astype(np.float32)
  D /= np.sqrt((D.astype(np.float64) ** 2).sum(axis=(1, 2, 3)))[
      :, None, None, None].astype(np.float32)
  return imgs, D, ((pad, pad), (pad, pad))


@pytest.mark.parametrize('name,k,c,s,height,width,stride,frame,tol', [
    # the default matrix-core route (test_split_modes_matrix_core_path, f16x3)
    ('x3', 11, 1, 32, 70, 93, 1, None, helpers.REL_TOL_F32),
    # scalar-tap kernels (test_unit_stride_specialisations)
    ('unit', 5, 2, 6, 70, 93, 1, None, helpers.REL_TOL_F32)])
def test_conv_inference(device, name, k, c, s, height, width, stride, frame,
                        tol):
  """imgs[1:] of a batch (8 bytes off for the one-channel 70x93 geometry), a
  kernel tensor one element into a buffer, and both skewed; default
  precision."""
  from analysis_transforms.convolutional import ista_fista as conv
  from utils import convolutions
  imgs, D, padding = _conv_case(3000 + k, k, s, height, width, 3, c, frame)
  geom = convolutions.geometry(torch.from_numpy(imgs[1:]),
                               torch.from_numpy(D), (stride, stride), padding)
  assert conv._resolve_precision(None, geom, False) == (
      'f16x3' if name == 'x3' else 'f32')
  eta = float(np.float32(sc_oracle.conv_stepsize(
      torch.from_numpy(D).double())))
  ref = sc_oracle.conv_ista_fista(
      torch.from_numpy(imgs[1:]).double(), torch.from_numpy(D).double(),
      (stride, stride), padding, 0.05, 8, stepsize=eta).numpy()
  Xd, Dd = helpers.to_dev(imgs, device), helpers.to_dev(D, device)
  view = Xd[1:]
  assert view.is_contiguous()
  assert view.data_ptr() % 16 == imgs[0].nbytes % 16
  if name == 'x3':                    # 90 x 113 padded floats per image
    assert view.data_ptr() % 16 == 8
  for label, X, Dk in (('imgs[1:]', view, Dd),
                       ('skewed kernels', Xd[1:].clone(), skewed(Dd)),
                       ('both', skewed(Xd[1:].clone()), skewed(Dd, 3))):
    codes = conv.run(X, Dk, (stride, stride), padding, 0.05, 8, stepsize=eta)
    helpers.assert_codes_match(codes.cpu().numpy(), ref, tol,
                               '%s, %s' % (name, label))
  assert torch.equal(Xd.cpu(), torch.from_numpy(imgs))


def test_conv_patch_route_against_the_reference_fixture(device):
  """conv.npz k8s4_ragged: 8x8 kernels at stride 4, the patch contractions.
  Skewed images, kernels, and both.  Gate:
  test_conv_gpu.py::test_inference_matches_reference."""
  from analysis_transforms.convolutional import ista_fista as conv
  g = helpers.load('conv')
  name = 'k8s4_ragged'
  imgs = helpers.to_dev(g[name + '_images_padded'], device)
  D = helpers.to_dev(g[name + '_dictionary'].copy(), device)
  stride = tuple(int(v) for v in g[name + '_stride'])
  pad = tuple(tuple(int(v) for v in row) for row in g[name + '_padding'])
  for label, X, Dk in (('images', skewed(imgs), D), ('kernels', imgs,
                                                     skewed(D)),
                       ('both', skewed(imgs, 3), skewed(D, 2))):
    for variant in ('ista', 'fista'):
      codes = conv.run(X, Dk, stride, pad, 0.05, 10, variant=variant)
      helpers.assert_codes_match(codes.cpu().numpy(),
                                 g['%s_codes_%s' % (name, variant)],
                                 helpers.REL_TOL_F32,
                                 '%s %s, skewed %s' % (name, variant, label))


def test_fc_update_lands_in_the_view(device):
  """sc_steepest_descent on a dictionary view and on skewed codes: the result
  is written in the view, the spare element is untouched.  Gate:
  REL_TOL_DICT."""
  from dict_update_rules.fully_connected import sc_steepest_descent
  b, n, s = 96, 100, 200
  X = helpers.gaussian_patches(31, b, n)
  D = helpers.unit_rows(32, s, n)
  rs = np.random.RandomState(33)
  C = (0.05 * rs.randn(b, s) * (rs.rand(b, s) < 0.1)).astype(np.float32)
  ref = torch.from_numpy(D).double()
  sc_oracle.fc_steepest_descent(torch.from_numpy(X).double(), ref,
                                torch.from_numpy(C).double(), stepsize=0.1)
  for label, skew_d, skew_c in (('dictionary', True, False),
                                ('codes', False, True), ('both', True, True)):
    Dv = helpers.to_dev(D.copy(), device)
    Cv = helpers.to_dev(C, device)
    Dv = skewed(Dv) if skew_d else Dv
    Cv = skewed(Cv) if skew_c else Cv
    sc_steepest_descent.run(helpers.to_dev(X, device), Dv, Cv, stepsize=0.1)
    torch.cuda.synchronize(device)
    err = helpers.rel_err(Dv.cpu().numpy(), ref.numpy())
    assert err < helpers.REL_TOL_DICT, (label, err)
    if skew_d:
      assert _spare_untouched(Dv)
      assert torch.equal(Dv.skew_buffer[1:].view(s, n), Dv)
    if skew_c:
      assert _spare_untouched(Cv)
      assert torch.equal(Cv.cpu(), torch.from_numpy(C))


def test_conv_update_lands_in_the_view(device):
  """The convolutional steepest-descent step on a kernel view.  Gate:
  REL_TOL_DICT."""
  from dict_update_rules.convolutional import sc_steepest_descent
  imgs, D, padding = _conv_case(41, 8, 16, 40, 52, 2, 1, 4)
  rs = np.random.RandomState(42)
  ch, cw = (48 - 8) // 4 + 1, (60 - 8) // 4 + 1
  C = (0.05 * rs.randn(2, 16, ch, cw) *
       (rs.rand(2, 16, ch, cw) < 0.2)).astype(np.float32)
  ref = torch.from_numpy(D).double()
  sc_oracle.conv_steepest_descent(torch.from_numpy(imgs).double(), ref,
                                  torch.from_numpy(C).double(), (4, 4),
                                  padding, stepsize=0.005)
  for label, skew_d, skew_c in (('kernels', True, False),
                                ('codes', False, True)):
    Dv = helpers.to_dev(D.copy(), device)
    Cv = helpers.to_dev(C, device)
    Dv = skewed(Dv) if skew_d else Dv
    Cv = skewed(Cv) if skew_c else Cv
    sc_steepest_descent.run(helpers.to_dev(imgs, device), Dv, Cv, (4, 4),
                            padding, stepsize=0.005)
    torch.cuda.synchronize(device)
    err = helpers.rel_err(Dv.cpu().numpy(), ref.numpy())
    assert err < helpers.REL_TOL_DICT, (label, err)
    if skew_d:
      assert _spare_untouched(Dv)


def test_row_transform_and_invertible_linear(device):
  """vtc_row_transform through vtc_hip.linalg and the ICA codes, n % 4 == 0
  (the 16-byte loads are gated on all three pointers).  Gates: 2e-6
  (test_zca_gpu.py) and 1e-6 (test_ica_gpu.py) against float64."""
  from vtc_hip import linalg
  from analysis_transforms.fully_connected import invertible_linear
  rs = np.random.RandomState(5)
  rows, n = 70, 64
  x = rs.randn(rows, n).astype(np.float32)
  off = rs.randn(n).astype(np.float32)
  q, _ = np.linalg.qr(rs.randn(n, n))
  m = (q * (1.0 + rs.rand(n))[None, :]).astype(np.float32)
  truth = (x - off[None, :]).astype(np.float64) @ m.astype(np.float64) + 0.25
  codes_truth = x.astype(np.float64) @ np.linalg.inv(m.astype(np.float64))
  for which in ('x', 'offsets', 'matrix'):
    t = {'x': helpers.to_dev(x, device), 'offsets': helpers.to_dev(off, device),
         'matrix': helpers.to_dev(m, device)}
    t[which] = skewed(t[which])
    y = linalg.row_transform(t['x'], t['offsets'], t['matrix'], 0.25)
    assert helpers.rel_err(y.cpu().numpy(), truth) <= 2e-6, which
    assert _spare_untouched(t[which])
  for which in ('x', 'matrix'):
    t = {'x': helpers.to_dev(x, device), 'matrix': helpers.to_dev(m, device)}
    t[which] = skewed(t[which])
    codes = invertible_linear.run(t['x'], t['matrix'])
    assert helpers.rel_err(codes.cpu().numpy(), codes_truth) <= 1e-6, which


@pytest.mark.parametrize('s,n', [(300, 200), (64, 64)])
def test_gram_and_lipschitz_step_on_a_dictionary_view(device, s, n):
  """vtc_hip.gram and the step size on a skewed dictionary.  Gates: the
  float32 summation bound s * 2^-24 * sum |terms| per Gram entry, and 3e-6 on
  the step (test_lipschitz_gpu.py, plugin against the library solver)."""
  import vtc_hip
  D = helpers.unit_rows(9 + s, s, n)
  view = skewed(helpers.to_dev(D, device))
  gram = vtc_hip.gram(view, transpose_a=True)
  d64 = D.astype(np.float64)
  truth = d64.T @ d64
  bound = s * 2.0 ** -24 * (np.abs(d64).T @ np.abs(d64))
  assert (np.abs(gram.cpu().numpy() - truth) <= bound).all()
  eta = vtc_hip.stepsize_from_gram(gram, view)
  ref = 1.0 / np.linalg.eigvalsh(truth)[-1]
  assert abs(float(eta) - ref) / ref < 3e-6
  assert _spare_untouched(view)
