"""ICA on the MI355X: invertible_linear.run against float64 truth and the
reference (tests/golden/ica_training.npz), training.ica.train_dictionary
against the reference's dictionaries up to the horizons where float32 and
float64 trajectories still agree, recovery of the mixing over a long run,
and the trainer's files, in-place update and singular-dictionary error.

ICA's update uses sign(codes): once a code near zero flips sign between two
runs, their dictionaries separate completely (tests/ica_data.py), so long
runs are judged by the Amari index, not against any other run."""
import pickle

import numpy as np
import pytest
import torch

import ica_data
from helpers import load

pytestmark = pytest.mark.gpu
K = ica_data.CODE_ROWS


@pytest.fixture(scope='module')
def golden():
  return load('ica_training')


def _params(**extra):
  p = {'num_epochs': 1, 'dictionary_update_algorithm': 'ica_natural_gradient',
       'dict_update_param_schedule': {
           0: {'stepsize': ica_data.STEPSIZE, 'num_iters': 1}},
       'stdout_print_interval': 1000000}
  p.update(extra)
  return p


# ---- invertible_linear ---------------------------------------------------
@pytest.mark.parametrize('ortho', [False, True])
@pytest.mark.parametrize('kappa', ica_data.KAPPAS)
@pytest.mark.parametrize('n', [64, 256])
def test_codes_match_float64_and_the_reference(device, golden, n, kappa,
                                               ortho):
  from analysis_transforms.fully_connected import invertible_linear
  x, d = ica_data.code_inputs(n, kappa)
  tag = 'codes_n%d_k%.0e' % (n, kappa)
  key = tag + ('_ortho' if ortho else '_inv')
  np.testing.assert_allclose(
      np.concatenate([ica_data.guard(x), ica_data.guard(d)]),
      golden[tag + '_guard'], rtol=1e-9)
  dg = torch.from_numpy(d).to(device)
  before = dg.clone()
  codes = invertible_linear.run(torch.from_numpy(x).to(device), dg,
                                orthonormal=ortho).cpu().numpy()
  assert torch.equal(dg, before)
  x64, d64 = x.astype(np.float64), d.astype(np.float64)
  truth = x64 @ (d64.T if ortho else np.linalg.inv(d64))
  assert ica_data.rel(codes, truth) <= 1e-6
  # the reference's float32 torch.inverse is itself up to 1.2e-4 from float64
  # at kappa = 1e4 (stored as <key>_dist): the gate against it allows that
  ref_dist = float(golden[key + '_dist'])
  assert ica_data.rel(codes[:K], golden[key]) <= 1e-5 + 1.1 * ref_dist


def test_run_refuses_bad_dictionaries(device):
  import vtc_hip
  from analysis_transforms.fully_connected import invertible_linear
  x = torch.zeros((4, 8), device=device)
  with pytest.raises(ValueError):
    invertible_linear.run(x, torch.zeros((8, 6), device=device))
  with pytest.raises(vtc_hip.VtcHipError):
    invertible_linear.run(x, torch.eye(8))
  with pytest.raises(torch.linalg.LinAlgError):
    invertible_linear.run(x, torch.zeros((8, 8), device=device))


# ---- train_dictionary against the reference ------------------------------
def _train(device, data, d0, params):
  from training import ica
  d = torch.from_numpy(np.array(d0)).to(device)
  log = ica.train_dictionary(torch.from_numpy(np.array(data)).to(device), d,
                             params)
  return d, log


@pytest.mark.parametrize('name', sorted(ica_data.CASES))
def test_train_dictionary_matches_the_reference(device, golden, name):
  n, nb, seed = ica_data.CASES[name]
  data, _ = ica_data.batches(n, nb, seed)
  d0 = ica_data.init_dictionary(n, seed)
  np.testing.assert_allclose(
      np.concatenate([ica_data.guard(data), ica_data.guard(d0)]),
      golden[name + '_guard'], rtol=1e-9)
  for steps in ica_data.HORIZONS[name]:
    d, _ = _train(device, data[:steps], d0, _params())
    got = d.cpu().numpy()
    truth = ica_data.truth_run(d0, data, {0: (ica_data.STEPSIZE, 1)}, steps)
    ref = golden['%s_step%d' % (name, steps)]
    assert ica_data.rel(got, ref) <= 1e-5, (steps, ica_data.rel(got, ref))
    assert ica_data.rel(got, truth) <= 1e-5


def test_schedule_values_take_effect_at_their_index(device, golden):
  n, nb, seed = ica_data.CASES['n64']
  data, _ = ica_data.batches(n, nb, seed)
  d0 = ica_data.init_dictionary(n, seed)
  params = _params(num_epochs=2, dict_update_param_schedule={
      0: {'stepsize': ica_data.STEPSIZE, 'num_iters': 1},
      3: {'stepsize': 0.05, 'num_iters': 2}})
  d, _ = _train(device, data[:3], d0, params)
  assert ica_data.rel(d.cpu().numpy(), golden['schedule']) <= 1e-5


# ---- recovery ------------------------------------------------------------
def test_long_run_recovers_the_mixing_and_repeats_bitwise(device):
  from training import ica
  n, nb, seed = ica_data.RECOVERY
  data, mixing = ica_data.batches(n, nb, seed)
  d0 = ica_data.init_dictionary(n, seed)
  start = ica_data.amari_index(d0, mixing)
  assert 0.25 < start < 0.35
  gpu_data = torch.from_numpy(data).to(device)
  finals = []
  for _ in range(2):
    d = torch.from_numpy(d0.copy()).to(device)
    ica.train_dictionary(gpu_data, d, _params(num_epochs=1000 // nb))
    finals.append(d.cpu().numpy())
  final = finals[0]
  assert np.all(np.isfinite(final))
  assert np.linalg.cond(final.astype(np.float64)) < 1e6
  assert ica_data.amari_index(final, mixing) <= 0.03
  assert np.array_equal(finals[0], finals[1])


# ---- files, in-place update, errors -------------------------------------
def test_checkpoints_yaml_metrics_and_in_place_update(device, tmp_path):
  from training import ica
  from training import sparse_coding
  n, nb, seed = ica_data.CASES['n64']
  data, _ = ica_data.batches(n, nb, seed)
  d0 = ica_data.init_dictionary(n, seed)
  d = torch.from_numpy(d0.copy()).to(device)
  logdir = tmp_path / 'ica_logs'
  params = _params(
      num_epochs=1, logging_folder_fullpath=logdir,
      checkpoint_schedule={0: None, 4: None},
      training_visualization_schedule={0: None, 3: None,
                                       'reshaped_kernel_size': (8, 8)},
      stdout_print_interval=2)
  batches = [torch.from_numpy(b) for b in data[:6]]   # host batches move over
  log = ica.train_dictionary(batches, d, params)
  # the dictionary object the caller passed was updated in place
  truth6 = ica_data.truth_run(d0, data, {0: (ica_data.STEPSIZE, 1)}, 6)
  assert ica_data.rel(d.cpu().numpy(), truth6) <= 1e-5
  # checkpoint i holds the dictionary before the update of iteration i
  with open(logdir / 'checkpoint_dictionary_iter_0', 'rb') as f:
    assert np.array_equal(pickle.load(f), d0)
  with open(logdir / 'checkpoint_dictionary_iter_4', 'rb') as f:
    ck4 = pickle.load(f)
  assert ck4.dtype == np.float32 and ck4.shape == (n, n)
  truth4 = ica_data.truth_run(d0, data, {0: (ica_data.STEPSIZE, 1)}, 4)
  assert ica_data.rel(ck4, truth4) <= 1e-5
  assert np.array_equal(
      sparse_coding.load_newest_dictionary_checkpoint(logdir), ck4)
  import yaml
  with open(logdir / 'training_params.yaml') as f:
    saved = yaml.unsafe_load(f)
  assert saved['dictionary_update_algorithm'] == 'ica_natural_gradient'
  assert saved['dict_update_param_schedule'][0]['stepsize'] == 0.1
  assert 'checkpoint_schedule' not in saved
  assert 'training_visualization_schedule' not in saved
  assert [it for it, _ in log] == [0, 3]
  for _, m in log:
    assert np.isfinite(m['Average pSNR of reconstructions'])
    assert m['Average pSNR of reconstructions'] > 20


def test_singular_initial_dictionary_raises(device):
  from training import ica
  n, nb, seed = ica_data.CASES['n64']
  data, _ = ica_data.batches(n, nb, seed)
  d0 = ica_data.init_dictionary(n, seed)
  d0[10] = d0[3]
  d = torch.from_numpy(d0).to(device)
  with pytest.raises(RuntimeError, match='iteration 0'):
    ica.train_dictionary(torch.from_numpy(data[:3]).to(device), d, _params())
