"""
Writes tests/golden/dataset.npz by running the REFERENCE's
create_patch_training_set (utils/dataset_generation.py:22-311) on the
synthetic Field_NW / Kodak_BW files of tests/dataset_data.py, and its
local_contrast_normalization / local_luminance_subtraction directly.

Development-container only: it imports the reference tree (absent on the GPU
machines) with the shims of oracle/make_golden.py.  Deterministic: re-running
it reproduces the fixture byte for byte.

  python tools/make_golden_dataset.py
"""
import pathlib
import sys
import tempfile

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'tests'))
sys.path.insert(0, str(REPO / 'oracle'))
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

import dataset_data  # noqa: E402
import make_golden  # noqa: E402


def main():
  ref = make_golden.import_reference()
  import importlib
  dg = importlib.import_module('utils.dataset_generation')
  conv = importlib.import_module('utils.convolutions')
  ip = ref.image_processing
  out = {}
  with tempfile.TemporaryDirectory() as tmp:
    files = dataset_data.write_files(pathlib.Path(tmp))
    for name, (dataset, num, patch, edge, ops, _, seed) in sorted(
        dataset_data.CASES.items()):
      extra = dataset_data.extra_params(name, files, conv.get_padding_amt)
      np.random.seed(seed)
      res = dg.create_patch_training_set(num, patch, edge, dataset, ops,
                                         extra)
      out[name + '_draws'] = np.random.randint(0, 2**31 - 1,
                                               size=dataset_data.DRAWS)
      out[name + '_keys'] = np.array(sorted(res))
      for key, val in res.items():
        if key == 'ZCA_parameters':
          out[name + '_zca_variances'] = np.asarray(
              val['PCA_axis_variances'], np.float32)
          out[name + '_zca_mean'] = np.float32(val['subtracted_mean'])
          continue
        out[name + '_shape_' + key] = np.array(val.shape)
        out[name + '_' + key] = dataset_data.stored(val).astype(np.float32)
  for name, (_, _, sigma) in sorted(dataset_data.DIRECT.items()):
    images = dataset_data.direct_images(name)
    for tag, fn in (('lcn', ip.local_contrast_normalization),
                    ('lls', ip.local_luminance_subtraction)):
      res = [fn(img, sigma, True) for img in images]
      out['g_%s_%s_out' % (name, tag)] = np.stack([r[0] for r in res])
      out['g_%s_%s_aux' % (name, tag)] = np.stack([r[1] for r in res])
  path = REPO / 'tests' / 'golden' / 'dataset.npz'
  np.savez_compressed(path, **out)
  print('wrote', path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
  main()
