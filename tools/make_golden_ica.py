"""
Writes tests/golden/ica_training.npz by running the REFERENCE's
analysis_transforms/fully_connected/invertible_linear.py run() and
training/ica.py train_dictionary (:128-240) on the inputs of tests/ica_data.py.

Development-container only: it imports the reference tree (absent on the GPU
machines) with the shims of oracle/make_golden.py.  ICA trajectories of a
float32 and a float64 run separate once a code near zero flips sign, so every
stored dictionary is also compared with the float64 statement of the same run
(ica_data.truth_run); the distance is stored and must be <= 2e-6 (otherwise
change the case's seed in ica_data.CASES).

  python tools/make_golden_ica.py
"""
import contextlib
import io
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'tests'))
sys.path.insert(0, str(REPO / 'oracle'))
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ica_data  # noqa: E402
import make_golden  # noqa: E402

SCHEDULE_CASE = {0: (ica_data.STEPSIZE, 1), 3: (0.05, 2)}
SCHEDULE_STEPS, SCHEDULE_EPOCHS = 3, 2   # 3 batches, 2 epochs: 6 iterations
LIMIT = 2e-6


def reference_train(ref_ica, d0, data, schedule, num_epochs):
  d = torch.from_numpy(np.array(d0, np.float32))
  params = {'num_epochs': num_epochs,
            'dictionary_update_algorithm': 'ica_natural_gradient',
            'dict_update_param_schedule': {
                k: {'stepsize': v[0], 'num_iters': v[1]}
                for k, v in schedule.items()}}
  with contextlib.redirect_stdout(io.StringIO()):
    ref_ica.train_dictionary(torch.from_numpy(np.array(data)), d, params)
  return d.numpy().copy()


def main():
  make_golden.import_reference()
  import importlib
  ref_lin = importlib.import_module(
      'analysis_transforms.fully_connected.invertible_linear')
  ref_ica = importlib.import_module('training.ica')
  torch.set_num_threads(8)
  out = {}
  k = ica_data.CODE_ROWS
  for n in (64, 256):
    for kappa in ica_data.KAPPAS:
      x, d = ica_data.code_inputs(n, kappa)
      tag = 'codes_n%d_k%.0e' % (n, kappa)
      out[tag + '_guard'] = np.concatenate([ica_data.guard(x),
                                            ica_data.guard(d)])
      for ortho in (False, True):
        c = ref_lin.run(torch.from_numpy(x), torch.from_numpy(d),
                        orthonormal=ortho).numpy()
        key = tag + ('_ortho' if ortho else '_inv')
        truth = x[:k].astype(np.float64) @ (
            d.T.astype(np.float64) if ortho
            else np.linalg.inv(d.astype(np.float64)))
        out[key] = c[:k]
        out[key + '_dist'] = np.float64(ica_data.rel(c[:k], truth))
        print('%s  reference vs float64 %.2e' % (key, out[key + '_dist']))
  one = {0: (ica_data.STEPSIZE, 1)}
  for name, (n, nb, seed) in ica_data.CASES.items():
    data, _ = ica_data.batches(n, nb, seed)
    d0 = ica_data.init_dictionary(n, seed)
    out[name + '_guard'] = np.concatenate([ica_data.guard(data),
                                           ica_data.guard(d0)])
    for steps in ica_data.HORIZONS[name]:
      d = reference_train(ref_ica, d0, data[:steps], one, 1)
      dist = ica_data.rel(d, ica_data.truth_run(d0, data, one, steps))
      print('%s step %3d  reference vs float64 %.2e' % (name, steps, dist))
      assert dist <= LIMIT, 'a sign tie was crossed: change the seed'
      out['%s_step%d' % (name, steps)] = d
      out['%s_step%d_dist' % (name, steps)] = np.float64(dist)
  # schedule case: n = 64, stepsize 0.05 and two update iterations from 3 on
  n, nb, seed = ica_data.CASES['n64']
  data, _ = ica_data.batches(n, nb, seed)
  d0 = ica_data.init_dictionary(n, seed)
  sub = data[:SCHEDULE_STEPS]
  d = reference_train(ref_ica, d0, sub, SCHEDULE_CASE, SCHEDULE_EPOCHS)
  steps = SCHEDULE_STEPS * SCHEDULE_EPOCHS
  dist = ica_data.rel(d, ica_data.truth_run(d0, sub, SCHEDULE_CASE, steps))
  print('schedule (%d steps)  reference vs float64 %.2e' % (steps, dist))
  assert dist <= LIMIT, 'a sign tie was crossed: change the seed'
  out['schedule'] = d
  out['schedule_dist'] = np.float64(dist)
  path = REPO / 'tests' / 'golden' / 'ica_training.npz'
  np.savez_compressed(path, **out)
  size = path.stat().st_size
  print('wrote', path, size, 'bytes')
  assert size < 1 << 20


if __name__ == '__main__':
  main()
