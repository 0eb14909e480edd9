"""create_patch_training_set and the local filters on the host side: the
separable statement of the reference's Gaussian filter against the fixture,
and every argument error raised before a file is read or a device touched.
No GPU needed."""
import numpy as np
import pytest

import dataset_data
import helpers
from utils import dataset_generation as dg
from utils import image_processing as ip

G = helpers.load('dataset')


def separable_filter(plane, sigma):
  """float64 statement: the normalised 1D factor of get_gaussian_filter_2d,
  applied along each axis of a symmetric-padded plane."""
  lower, taps = ip.gaussian_window(sigma)
  v = np.arange(lower, lower + taps, dtype=np.float64)
  g = np.exp(-0.5 * v * v / sigma**2)
  g /= g.sum()
  r = -lower
  p = np.pad(plane.astype(np.float64), r, mode='symmetric')
  h, w = plane.shape
  rows = sum(g[k] * p[:, k:k + w] for k in range(taps))
  return sum(g[k] * rows[k:k + h, :] for k in range(taps))


def lls(img, sigma):
  aux = np.stack([separable_filter(img[:, :, c], sigma)
                  for c in range(img.shape[2])], axis=2).astype(np.float32)
  return img - aux, aux


def lcn(img, sigma):
  sq = img * img
  v = np.stack([separable_filter(sq[:, :, c], sigma)
                for c in range(img.shape[2])], axis=2).astype(np.float32)
  v[v == 0] = 1.
  aux = np.sqrt(v)
  return img / aux, aux


@pytest.mark.parametrize('name', sorted(dataset_data.DIRECT))
@pytest.mark.parametrize('tag', ['lcn', 'lls'])
def test_separable_statement_reproduces_the_reference(name, tag):
  sigma = dataset_data.DIRECT[name][2]
  images = dataset_data.direct_images(name)
  fn = lcn if tag == 'lcn' else lls
  res = [fn(img, sigma) for img in images]
  out = np.stack([r[0] for r in res])
  aux = np.stack([r[1] for r in res])
  ref_out = G['g_%s_%s_out' % (name, tag)]
  ref_aux = G['g_%s_%s_aux' % (name, tag)]
  assert out.shape == ref_out.shape
  assert helpers.rel_err(aux, ref_aux) <= 1e-7
  assert helpers.rel_err(out, ref_out) <= 1e-7


def test_symmetric_fold_of_windows_wider_than_the_image():
  # the period-2n fold the kernel uses equals np.pad(mode='symmetric')
  for n, r in ((6, 6), (9, 6), (3, 8), (4, 8), (1, 5)):
    idx = np.arange(-r, n + r)
    m = np.mod(idx, 2 * n)
    fold = np.where(m < n, m, 2 * n - 1 - m)
    expect = np.pad(np.arange(n), r, mode='symmetric')
    assert np.array_equal(fold, expect)


def test_gaussian_window_follows_the_reference_rule():
  assert ip.gaussian_window(2) == (-4, 9)
  assert ip.gaussian_window(8) == (-16, 33)
  assert ip.gaussian_window(1.1) == (-2, 5)     # window 5.4
  for bad in (1.25, 0.25, 0, -1, float('nan'), 'two', None):
    with pytest.raises(ValueError):
      ip.gaussian_window(bad)


FIELD = {'filepath': '/nonexistent/field.mat'}


@pytest.mark.parametrize('ops, extra, exc', [
    (['standardize_data_range'], FIELD, AssertionError),        # no 'patch'
    (['patch', 'pad'], dict(FIELD, flatten_patches=False), AssertionError),
    (['local_contrast_normalization', 'patch'], FIELD, AssertionError),
    (['local_luminance_subtraction', 'patch'], FIELD, AssertionError),
    (['patch', 'standardize_data_range'], FIELD, AssertionError),
    (['standardize_data_range', 'standardize_data_range', 'patch'], FIELD,
     AssertionError),
    (['patch', 'whiten_center_surround'], FIELD, KeyError),
    (['patch', 'local_contrast_normalization'],
     dict(FIELD, lcn_filter_sigma=2), KeyError),
    (['patch', 'local_luminance_subtraction'],
     dict(FIELD, lls_filter_sigma=2), KeyError),
    (['whiten_ZCA', 'patch'], FIELD, KeyError),
    (['center_each_component', 'patch'], FIELD, KeyError),
    (['normalize_component_variance', 'patch'], FIELD, KeyError),
    (['center_each_patch', 'patch'], FIELD, KeyError),
    (['pad', 'patch'], dict(FIELD, padding=((1, 1), (1, 1)),
                            flatten_patches=False), KeyError),
    (['patch', 'pad'], dict(FIELD, padding=((1, 1), (1, 1))), KeyError),
    (['patch', 'sharpen'], FIELD, KeyError),
    (['local_contrast_normalization', 'patch'],
     dict(FIELD, lcn_filter_sigma=1.25), ValueError),           # even window
    (['local_luminance_subtraction', 'patch'],
     dict(FIELD, lls_filter_sigma=0.75), ValueError),
])
def test_argument_errors_come_before_any_work(ops, extra, exc):
  # the file does not exist and there is no GPU: the error must come first
  with pytest.raises(exc):
    dg.create_patch_training_set(10, (8, 8), 0, 'Field_NW', ops, extra)


def test_dataset_name_errors():
  ops = ['patch']
  with pytest.raises(KeyError):
    dg.create_patch_training_set(10, (8, 8), 0, 'Imagenet', ops, FIELD)
  with pytest.raises(KeyError):
    dg.create_patch_training_set(10, (8, 8), 0, 'Field_NW', ops, {})
  with pytest.raises(NotImplementedError):
    dg.create_patch_training_set(10, (8, 8), 0, 'Kodak', ops, FIELD)


def test_kodak_bw_file_is_read_without_running_code(tmp_path):
  import pickle

  class Payload:
    def __reduce__(self):
      return (print, ('never printed',))
  path = tmp_path / 'evil.p'
  path.write_bytes(pickle.dumps([Payload()]))
  with pytest.raises(pickle.UnpicklingError):
    dg.create_patch_training_set(10, (8, 8), 0, 'Kodak_BW', ['patch'],
                                 {'filepath': str(path)})


def test_new_workspace_queries_are_host_only():
  import vtc_hip
  lib = vtc_hip.load_library()
  # LDS route up to radius 16: no workspace
  assert lib.vtc_local_normalize_workspace_bytes(64, 512, 512, 1, 8.0) == 0
  # wider: one float64 plane per image channel
  assert lib.vtc_local_normalize_workspace_bytes(2, 30, 40, 3, 9.0) == (
      8 * 2 * 30 * 40 * 3)
  assert lib.vtc_column_moments_workspace_bytes(131072, 256) >= 16 * 256
  assert lib.vtc_column_moments_workspace_bytes(0, 256) == 0


def test_new_entry_points_refuse_bad_arguments_without_the_gpu():
  import vtc_hip
  lib = vtc_hip.load_library()
  rc = lib.vtc_local_normalize(None, None, None, 1, 8, 8, 1, 2.0, 0, None, 0,
                               None)
  assert rc == vtc_hip.ERR_INVALID_ARGUMENT
  assert b'null' in lib.vtc_last_error()
  fake = 1 << 20   # never dereferenced: the checks fail first
  rc = lib.vtc_local_normalize(fake, fake + 64, fake + 128, 1, 8, 8, 1, 1.25,
                               0, None, 0, None)
  assert rc == vtc_hip.ERR_INVALID_ARGUMENT
  assert b'even' in lib.vtc_last_error()
  rc = lib.vtc_local_normalize(fake, fake + 64, fake + 128, 1, 8, 8, 1, 70.0,
                               0, None, 0, None)
  assert rc == vtc_hip.ERR_UNSUPPORTED
  rc = lib.vtc_local_normalize(fake, fake + 64, fake + 128, 1, 0, 8, 1, 2.0,
                               0, None, 0, None)
  assert rc == vtc_hip.ERR_INVALID_ARGUMENT
  assert lib.vtc_column_moments(None, 0, 4, 4, None, None, None, 0,
                                None) == vtc_hip.ERR_INVALID_ARGUMENT
  assert lib.vtc_column_apply(fake, 0, 4, 4, 7, fake, fake,
                              None) == vtc_hip.ERR_INVALID_ARGUMENT
  assert lib.vtc_row_center(fake, 2, 4, 4, fake, None,
                            None) == vtc_hip.ERR_INVALID_ARGUMENT


def test_one_output_dset():
  import torch
  t = torch.arange(12.).reshape(4, 3)
  d = dg.OneOutputDset(t)
  assert len(d) == 4 and torch.equal(d[2], t[2])
