"""
ICA dictionary learning on MI355X: the reference's training/ica.py
(train_dictionary at :9-240) with its parameter dictionary and semantics.

Each step is inverse -> codes -> natural-gradient update, all in HIP:
vtc_mat_inverse (float64 LU, vtc_hip.linalg.mat_inverse), vtc_row_transform
(invertible_linear.apply_filter) and ica_natural_gradient.run
(vtc_ica_moment / vtc_ica_apply).  The reference's torch.inverse raises on a
singular dictionary; here each step's inverse status stays on the device, in
a ring of status rows that is read back at every print interval, checkpoint,
visualisation iteration, when the ring is full and at the end of training.
A singular step then raises RuntimeError naming the first such iteration.

TensorBoard summaries and dictionary figures are not drawn: at the
'training_visualization_schedule' iterations the reference's scalar, the
average reconstruction pSNR of the batch, is appended to the returned metrics
log as (iteration, {'Average pSNR of reconstructions': value}), the way
training.sparse_coding keeps TrainingStep.metrics_log.
"""
import pickle
import time

import numpy as np
import torch

import vtc_hip
from vtc_hip import linalg
from vtc_hip import parallel

_STATUS_RING = 1024   # steps between forced reads of the inverse status


class _StatusRing(object):
  """Device status rows of consecutive steps' inverses; check() reads them
  back (one host synchronisation) and raises for the first singular one."""

  def __init__(self, device):
    self.rows = torch.empty((_STATUS_RING, 2), dtype=torch.int32,
                            device=device)
    self.first_iter = 0
    self.used = 0

  def next_row(self, iteration):
    if self.used == _STATUS_RING:
      self.check()
    if self.used == 0:
      self.first_iter = iteration
    row = self.rows[self.used]
    self.used += 1
    return row

  def check(self):
    if self.used == 0:
      return
    seen = self.rows[:self.used].cpu().numpy()
    self.used = 0
    bad = np.nonzero(seen[:, 0] != 1)[0]
    if len(bad):
      it = self.first_iter + int(bad[0])
      pivot = int(seen[bad[0], 1])
      raise RuntimeError(
          'ICA training: the dictionary at iteration %d is singular or not '
          'finite (%s); its inverse, and every update after it, is not '
          'meaningful' % (it, 'first bad pivot %d' % pivot if pivot >= 0
                          else 'non-finite entries'))


def _average_recon_psnr(batch_images, codes, dictionary):
  """log_training_progress's scalar (reference :73-84): per-sample pSNR of
  codes @ dictionary against the batch, signal range estimated from the
  batch, infinite values skipped, averaged."""
  batch_images_np = batch_images.cpu().numpy()
  batch_sig_mag = np.max(batch_images_np) - np.min(batch_images_np)
  recons = torch.mm(codes, dictionary).cpu().numpy()
  recon_psnr = []
  for b_idx in range(recons.shape[0]):
    mse = np.mean(np.square(batch_images_np[b_idx, :] - recons[b_idx, :]))
    if mse != 0:
      recon_psnr.append(10. * np.log10((batch_sig_mag ** 2) / mse))
  return np.mean(recon_psnr)


def train_dictionary(image_dataset, init_dictionary, all_params):
  """
  Train an ICA dictionary; `init_dictionary` is updated IN PLACE (the
  reference does not copy it).

  image_dataset : iterable of (b, n) float32 batches (a (k, b, n) tensor or a
      torch DataLoader); a batch on another device is moved to the
      dictionary's.
  init_dictionary : (n, n) float32 HIP device tensor.
  all_params : the reference's dictionary.  Mandatory: 'num_epochs',
      'dictionary_update_algorithm' ('ica_natural_gradient' only),
      'dict_update_param_schedule' (iteration -> {'stepsize', 'num_iters'},
      index 0 present).  Optional: 'checkpoint_schedule',
      'training_visualization_schedule' (non-integer keys such as
      'reshaped_kernel_size' are tolerated), 'logging_folder_fullpath'
      (pathlib.Path), 'stdout_print_interval' (default 1000),
      'reshaped_kernel_size' (popped, as the reference does; only its figures
      use it).

  Returns the metrics log, a list of (iteration, {'Average pSNR of
  reconstructions': float}) at the visualisation iterations.  Raises
  RuntimeError, at the latest before returning, if the dictionary of some
  iteration was singular.
  """
  assert 0 in all_params['dict_update_param_schedule']
  assert init_dictionary.size(0) == init_dictionary.size(1)  # critically sample
  num_epochs = all_params['num_epochs']
  dict_update_alg = all_params['dictionary_update_algorithm']
  dict_update_param_schedule = all_params['dict_update_param_schedule']
  assert dict_update_alg in ['ica_natural_gradient']
  dictionary = vtc_hip.require_device_tensor(init_dictionary,
                                             'init_dictionary')
  assert dictionary.is_contiguous(), 'the dictionary is updated in place'

  logging_path = None
  if 'logging_folder_fullpath' in all_params:
    assert type(all_params['logging_folder_fullpath']) != str, (
        'should be pathlib.Path')
    logging_path = all_params['logging_folder_fullpath']
    if ('checkpoint_schedule' in all_params or
        'training_visualization_schedule' in all_params):
      if logging_path.exists():
        print('-------\n',
              'Warning, saving checkpoints and/or tensorboard logs into ',
              'existing, directory. Will overwrite existing files\n-------')
      else:
        logging_path.mkdir(parents=True)
  ckpt_sched = all_params.get('checkpoint_schedule')
  trn_vis_sched = all_params.get('training_visualization_schedule')
  if trn_vis_sched is not None and 'reshaped_kernel_size' in all_params:
    all_params.pop('reshaped_kernel_size')
  if (ckpt_sched is not None or trn_vis_sched is not None) and (
      parallel.rank() == 0):
    import yaml
    saved_training_params = {
        k: all_params[k] for k in all_params if k not in
        ['checkpoint_schedule', 'training_visualization_schedule']}
    with open(logging_path / 'training_params.yaml', 'w') as f:
      yaml.dump(saved_training_params, f)
  print_interval = all_params.get('stdout_print_interval', 1000)

  from analysis_transforms.fully_connected import invertible_linear
  from dict_update_rules.fully_connected import ica_natural_gradient

  n = dictionary.shape[0]
  status = _StatusRing(dictionary.device)
  metrics_log = []
  starttime = time.time()
  total_iter_idx = 0
  for epoch_idx in range(num_epochs):
    for batch_images in image_dataset:
      if total_iter_idx % print_interval == 0:
        status.check()
        print('Iteration', total_iter_idx, 'complete')
        print('Time elapsed:', '{:.1f}'.format(time.time() - starttime),
              'seconds')
        print('-----')

      if dictionary.device != batch_images.device:
        batch_images = batch_images.to(dictionary.device)
      batch_images = vtc_hip.require_device_tensor(
          batch_images, 'batch_images').contiguous()
      if batch_images.dim() != 2 or batch_images.shape[1] != n:
        raise ValueError('batches must be (b, %d), got shape %s'
                         % (n, tuple(batch_images.shape)))

      # code inference: the inverse's status stays on the device
      filter_matrix, _ = linalg.mat_inverse(
          dictionary, status=status.next_row(total_iter_idx))
      codes = invertible_linear.apply_filter(batch_images, filter_matrix)

      if ckpt_sched is not None and total_iter_idx in ckpt_sched:
        status.check()
        if parallel.rank() == 0:
          with open(logging_path / ('checkpoint_dictionary_iter_' +
                                    str(total_iter_idx)), 'wb') as f:
            pickle.dump(dictionary.cpu().numpy(), f)
      if trn_vis_sched is not None and total_iter_idx in trn_vis_sched:
        status.check()
        metrics_log.append((total_iter_idx, {
            'Average pSNR of reconstructions': _average_recon_psnr(
                batch_images, codes, dictionary)}))

      if total_iter_idx in dict_update_param_schedule:
        d_upd_stp = dict_update_param_schedule[total_iter_idx]['stepsize']
        d_upd_niters = dict_update_param_schedule[total_iter_idx]['num_iters']
      ica_natural_gradient.run(dictionary, codes, d_upd_stp, d_upd_niters)

      total_iter_idx += 1
    print("Epoch", epoch_idx, "finished")
  status.check()
  return metrics_log
