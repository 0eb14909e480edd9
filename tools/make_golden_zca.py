"""
Writes tests/golden/zca.npz by running the REFERENCE's whiten_ZCA /
unwhiten_ZCA (utils/image_processing.py:338-460) and training/pca.py
train_dictionary on the inputs of tests/zca_data.py.

Development-container only: it imports the reference tree (absent on the GPU
machines) with the shims of oracle/make_golden.py.  Deterministic: re-running
it reproduces the fixture byte for byte.

  python tools/make_golden_zca.py
"""
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'tests'))
sys.path.insert(0, str(REPO / 'oracle'))
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden  # noqa: E402
import zca_data  # noqa: E402


def main():
  ref = make_golden.import_reference()
  import importlib
  ref_pca = importlib.import_module('training.pca')
  ip = ref.image_processing
  out = {}
  k = zca_data.STORED_ROWS
  for name in zca_data.CASES:
    est, held = zca_data.case_data(name)
    white, params = ip.whiten_ZCA(est)
    pre = ip.whiten_ZCA(held, params)
    unwhite = ip.unwhiten_ZCA(pre[:k], params)
    out[name + '_guard_est'] = zca_data.guard(est)
    out[name + '_guard_held'] = zca_data.guard(held)
    out[name + '_head_est'] = est[:2]
    out[name + '_head_held'] = held[:2]
    out[name + '_white'] = white[:k]
    out[name + '_basis'] = params['PCA_basis'].astype(np.float32)
    out[name + '_variances'] = params['PCA_axis_variances'].astype(np.float32)
    out[name + '_mean'] = np.float32(params['subtracted_mean'])
    out[name + '_pre'] = pre[:k]
    out[name + '_unwhite'] = unwhite
    # how far the reference is from the float64 statement (printed only)
    t_white, t_params = zca_data.truth_estimate(est)
    lam = t_params['PCA_axis_variances']
    print('%-5s estimating %.2e  precomputed %.2e  unwhiten %.2e  '
          'max|dw|/w_max %.2e  round trip %.2e  w in [%.1e, %.1e]' % (
              name, zca_data.rel(white[:k], t_white[:k]),
              zca_data.rel(pre[:k], zca_data.truth_whiten(held[:k], params)),
              zca_data.rel(unwhite, zca_data.truth_unwhiten(pre[:k], params)),
              np.abs(params['PCA_axis_variances'] - lam).max() / lam[0],
              zca_data.rel(ip.unwhiten_ZCA(white, params), est),
              lam[-1], lam[0]))
  x = zca_data.pca_data()
  out['pca_dictionary'] = ref_pca.train_dictionary(
      torch.from_numpy(x)).numpy().astype(np.float32)
  path = REPO / 'tests' / 'golden' / 'zca.npz'
  np.savez_compressed(path, **out)
  print('wrote', path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
  main()
