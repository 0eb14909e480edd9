"""create_patch_training_set, the local filters and the patch statistics on
the device against the reference's own outputs (tests/golden/dataset.npz,
tools/make_golden_dataset.py)."""
import numpy as np
import pytest
import torch

import dataset_data
import helpers
from utils import convolutions
from utils import dataset_generation as dg
from utils import image_processing as ip

pytestmark = pytest.mark.gpu
G = helpers.load('dataset')
REL = 1e-6


@pytest.fixture(scope='module')
def files(tmp_path_factory):
  return dataset_data.write_files(tmp_path_factory.mktemp('datasets'))


def run_case(name, files):
  dataset, num, patch, edge, ops, _, seed = dataset_data.CASES[name]
  extra = dataset_data.extra_params(name, files, convolutions.get_padding_amt)
  np.random.seed(seed)
  res = dg.create_patch_training_set(num, patch, edge, dataset, ops, extra)
  torch.cuda.synchronize()
  draws = np.random.randint(0, 2**31 - 1, size=dataset_data.DRAWS)
  return res, draws


@pytest.mark.parametrize('name', sorted(dataset_data.CASES))
def test_case_matches_the_reference(name, files, device):
  res, draws = run_case(name, files)
  assert sorted(res) == sorted(G[name + '_keys'].tolist())
  assert np.array_equal(draws, G[name + '_draws'])
  for key, val in res.items():
    if key == 'ZCA_parameters':
      lam = G[name + '_zca_variances']
      w = val['PCA_axis_variances'].cpu().numpy()
      assert np.abs(w - lam).max() <= 1e-6 * lam[0]
      assert abs(float(val['subtracted_mean'].cpu()) -
                 float(G[name + '_zca_mean'])) <= 1e-6
      continue
    assert val.is_cuda and val.dtype == torch.float32, key
    assert tuple(val.shape) == tuple(G[name + '_shape_' + key]), key
    ours = dataset_data.stored(val.cpu().numpy())
    ref = G[name + '_' + key]
    if name == 'a':
      assert np.array_equal(ours, ref), key
    elif name == 'd' and key == 'patches':
      assert helpers.rel_err(ours, ref) <= 3e-5, key
    else:
      assert helpers.rel_err(ours, ref) <= REL, (key, helpers.rel_err(
          ours, ref))


@pytest.mark.parametrize('name', ['c', 'd'])
def test_repeated_call_is_bitwise_identical(name, files, device):
  first, _ = run_case(name, files)
  second, _ = run_case(name, files)
  for key, val in first.items():
    if key == 'ZCA_parameters':
      for k, v in val.items():
        assert torch.equal(v, second[key][k]), k
    else:
      assert torch.equal(val, second[key]), key


def test_image_list_and_stack_inputs(files, device):
  """The extension: the same images as a device stack give the reference's
  result (case b)."""
  import scipy.io
  raw = scipy.io.loadmat(files['Field_NW'])['IMAGESr'].astype('float32')
  stack = torch.from_numpy(np.ascontiguousarray(
      np.transpose(raw, (2, 0, 1))[..., None])).to(device)
  _, num, patch, edge, ops, _, seed = dataset_data.CASES['b']
  np.random.seed(seed)
  res = dg.create_patch_training_set(num, patch, edge, stack, ops)
  np.random.seed(seed)
  res2 = dg.create_patch_training_set(num, patch, edge, list(stack), ops)
  assert helpers.rel_err(res['patches'].cpu().numpy(), G['b_patches']) <= REL
  assert torch.equal(res['patches'], res2['patches'])


@pytest.mark.parametrize('name', sorted(dataset_data.DIRECT))
@pytest.mark.parametrize('tag', ['lcn', 'lls'])
def test_local_filters_match_the_reference(name, tag, device):
  sigma = dataset_data.DIRECT[name][2]
  images = torch.from_numpy(dataset_data.direct_images(name)).to(device)
  fn = (ip.local_contrast_normalization if tag == 'lcn'
        else ip.local_luminance_subtraction)
  out, aux = fn(images, sigma, True)
  ref_out = G['g_%s_%s_out' % (name, tag)]
  ref_aux = G['g_%s_%s_aux' % (name, tag)]
  assert helpers.rel_err(aux.cpu().numpy(), ref_aux) <= REL
  assert helpers.rel_err(out.cpu().numpy(), ref_out) <= REL
  # a single image equals the same image inside the stack
  last = fn(images[-1].clone(), sigma, True)
  assert torch.equal(last[0], out[-1]) and torch.equal(last[1], aux[-1])
  assert torch.equal(fn(images, sigma), out)


def test_statistics_against_float64(device):
  rs = np.random.RandomState(5)
  x = (3.0 + 0.01 * rs.randn(3001, 70)).astype(np.float32)
  xd = torch.from_numpy(x).to(device)
  x64 = x.astype(np.float64)
  cen, means = ip.center_each_component(xd)
  assert helpers.rel_err(means.cpu().numpy(), x64.mean(axis=0)) <= 1e-7
  assert helpers.rel_err(cen.cpu().numpy(), x64 - x64.mean(axis=0)) <= 1e-5
  nrm, var = ip.normalize_component_variance(xd)
  assert helpers.rel_err(var.cpu().numpy(), x64.var(axis=0)) <= 1e-6
  assert helpers.rel_err(nrm.cpu().numpy(),
                         x64 / np.sqrt(x64.var(axis=0))) <= 1e-6
  smp, rmeans = ip.center_each_sample(xd)
  assert helpers.rel_err(rmeans.cpu().numpy(), x64.mean(axis=1)) <= 1e-7
  assert helpers.rel_err(smp.cpu().numpy(),
                         x64 - x64.mean(axis=1)[:, None]) <= 1e-5
  # bitwise reproducible
  assert torch.equal(ip.normalize_component_variance(xd)[1], var)


def test_statistics_accept_uint8(device):
  rs = np.random.RandomState(6)
  x = rs.randint(0, 256, size=(500, 33)).astype(np.uint8)
  xd = torch.from_numpy(x).to(device)
  xf = torch.from_numpy(x.astype(np.float32)).to(device)
  for fn in (ip.center_each_component, ip.normalize_component_variance,
             ip.center_each_sample):
    a, b = fn(xd)
    c, d = fn(xf)
    assert a.dtype == torch.float32
    assert torch.equal(a, c) and torch.equal(b, d)
  _, m = ip.center_each_component(xd)
  assert helpers.rel_err(m.cpu().numpy(), x.mean(axis=0)) <= 1e-7
