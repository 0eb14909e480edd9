"""Inputs and cases of the create_patch_training_set tests
(tests/golden/dataset.npz is written by tools/make_golden_dataset.py from the
same functions).

Images are synthetic 1/f-spectrum fields drawn from
numpy.random.RandomState(seed): a Field_NW-like float32 stack IMAGESr
(h, w, count) with the dataset's odd range (about -3 .. 6), and a ragged
Kodak_BW-like list of uint8 images of 40x56 and 56x40."""
import pickle

import numpy as np

FIELD_SEED, KODAK_SEED = 21, 22
FIELD_SHAPE = (48, 64, 4)             # IMAGESr: (h, w, count)
KODAK_SHAPES = [(40, 56), (56, 40), (40, 56), (56, 40), (40, 56)]
STORED_ROWS = 160   # rows of a large reference output kept in the fixture
DRAWS = 4           # np.random.randint draws recorded after each call

# name -> (dataset, num_samples, patch_dimensions, edge_buffer, ops,
#          extra_params without 'filepath', numpy seed before the call)
CASES = {
    'a': ('Field_NW', 160, (8, 8), 4, ['patch'], {}, 101),
    'b': ('Field_NW', 160, (8, 8), 4,
          ['standardize_data_range', 'whiten_center_surround', 'patch'], {},
          102),
    'c': ('Field_NW', 1000, (8, 8), 4,
          ['standardize_data_range', 'local_luminance_subtraction',
           'local_contrast_normalization', 'patch', 'center_each_component',
           'normalize_component_variance', 'center_each_patch'],
          {'lls_filter_sigma': 2, 'lcn_filter_sigma': 5}, 103),
    'd': ('Kodak_BW', 1200, (8, 12), 3,
          ['standardize_data_range', 'patch', 'whiten_ZCA'], {}, 104),
    'e': ('Field_NW', 96, (8, 8), 4,
          ['standardize_data_range', 'whiten_center_surround', 'patch',
           'pad'], {'flatten_patches': False}, 105),
    'f': ('Kodak_BW', 160, (8, 8), 2, ['patch', 'center_each_component'], {},
          106),
}
# case e: padding for 8x8 patches, 6x6 kernels at stride 2 (get_padding_amt)
E_KERNEL, E_STRIDE = 6, 2

# case g: direct LCN / LLS calls.  name -> (images (count, h, w, c) seed and
# shape, sigma).  'small' is smaller than the window (r = 2 sigma); 'wide' is
# past the LDS tile's radius.
DIRECT = {
    'stack': (31, (3, 24, 70, 2), 2),
    'small': (32, (1, 6, 9, 1), 3),
    'tiny': (33, (1, 3, 4, 1), 4),
    'wide': (34, (2, 30, 40, 1), 9),
}


def one_over_f(rs, count, h, w):
  noise = rs.randn(count, h, w)
  fy = np.fft.fftfreq(h)[:, None]
  fx = np.fft.fftfreq(w)[None, :]
  f = np.sqrt(fy * fy + fx * fx)
  f[0, 0] = 1.0 / max(h, w)
  return np.real(np.fft.ifft2(np.fft.fft2(noise) / f))


def field_images():
  """IMAGESr (h, w, count) float32, values in about [-3.2, 6.4]."""
  h, w, count = FIELD_SHAPE
  img = one_over_f(np.random.RandomState(FIELD_SEED), count, h, w)
  img = img / np.abs(img).max()
  scale = np.linspace(3.0, 6.4, count)[:, None, None]
  return np.transpose(img * scale, (1, 2, 0)).astype(np.float32)


def kodak_images():
  rs = np.random.RandomState(KODAK_SEED)
  out = []
  for h, w in KODAK_SHAPES:
    img = one_over_f(rs, 1, h, w)[0]
    img = (img - img.min()) / (img.max() - img.min())
    out.append(np.round(255 * img).astype(np.uint8))
  return out


def direct_images(name):
  seed, shape, _ = DIRECT[name]
  rs = np.random.RandomState(seed)
  return (0.5 + rs.rand(*shape)).astype(np.float32)


def write_files(directory):
  """The two dataset files, as the reference's loaders read them."""
  import scipy.io
  field = directory / 'field_nw.mat'
  scipy.io.savemat(str(field), {'IMAGESr': field_images()})
  kodak = directory / 'kodak_bw.p'
  with open(kodak, 'wb') as f:
    pickle.dump(kodak_images(), f)
  return {'Field_NW': str(field), 'Kodak_BW': str(kodak)}


def extra_params(name, files, get_padding_amt):
  dataset, _, patch, _, ops, extra, _ = CASES[name]
  extra = dict(extra, filepath=files[dataset])
  if 'pad' in ops:
    extra['padding'] = (get_padding_amt(patch[0], E_KERNEL, E_STRIDE),
                        get_padding_amt(patch[1], E_KERNEL, E_STRIDE))
  return extra


def stored(a):
  """What the fixture keeps of one output: the first STORED_ROWS rows."""
  return np.asarray(a)[:STORED_ROWS]
