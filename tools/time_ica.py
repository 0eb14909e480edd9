"""Times ICA on one device with HIP events (medians of repeated runs):
vtc_mat_inverse at n = 64, 192, 256; one full ICA step (inverse -> codes ->
natural-gradient update) at b = 250 with n = 64 and 256, its phases, and the
same step written in torch (torch.linalg.inv, mm, sign) on the same GPU.

  python3 tools/time_ica.py  > profiles/ica_training.txt
"""
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent /
                       'vision-transform-codes_amd'))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent /
                       'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ica_data  # noqa: E402
from analysis_transforms.fully_connected import invertible_linear  # noqa
from dict_update_rules.fully_connected import ica_natural_gradient  # noqa
from vtc_hip import linalg  # noqa: E402

dev = torch.device('cuda:0')
B = ica_data.BATCH


def median_ms(fn, reps):
  for _ in range(3):
    fn()
  times = []
  for _ in range(reps):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    times.append(a.elapsed_time(b))
  return float(np.median(times)), float(np.min(times)), float(np.max(times))


def hip_step(x, d, status):
  d_inv, _ = linalg.mat_inverse(d, status=status)
  codes = invertible_linear.apply_filter(x, d_inv)
  ica_natural_gradient.run(d, codes, 1e-6, 1)


def torch_step(x, d, eye):
  codes = torch.mm(x, torch.linalg.inv(d))
  d.add_(1e-6 * torch.mm(torch.mm(codes.t(), torch.sign(codes)) / B - eye,
                         d))


def main():
  print('device: %s' % torch.cuda.get_device_name(dev))
  print('HIP-event medians [min, max] in ms')
  for n in (64, 192, 256):
    a = torch.from_numpy(ica_data.conditioned(n, 1e2, n)).to(dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    ms = median_ms(lambda: linalg.mat_inverse(a, status=status), 50)
    lib_ms = median_ms(lambda: torch.linalg.inv(a), 50)
    print('vtc_mat_inverse n = %3d  %8.4f [%8.4f, %8.4f]   '
          'torch.linalg.inv (f32) %8.4f [%8.4f, %8.4f]' % ((n,) + ms + lib_ms))
  for n in (64, 256):
    data, _ = ica_data.batches(n, 4, ica_data.CASES['n%d' % n][2])
    x = torch.from_numpy(data[0]).to(dev)
    d0 = torch.from_numpy(ica_data.init_dictionary(n, 1)).to(dev)
    d = d0.clone()
    status = torch.empty(2, dtype=torch.int32, device=dev)
    eye = torch.eye(n, device=dev)
    d_inv, _ = linalg.mat_inverse(d, status=status)
    codes = invertible_linear.apply_filter(x, d_inv)
    inv_ms = median_ms(lambda: linalg.mat_inverse(d, status=status), 50)
    code_ms = median_ms(lambda: invertible_linear.apply_filter(x, d_inv), 50)
    upd_ms = median_ms(
        lambda: ica_natural_gradient.run(d, codes, 1e-6, 1), 50)
    step_ms = median_ms(lambda: hip_step(x, d, status), 50)
    d.copy_(d0)
    torch_ms = median_ms(lambda: torch_step(x, d, eye), 50)
    print('ICA step n = %3d b = %d: HIP %8.4f [%8.4f, %8.4f]  '
          '(inverse %.4f, codes %.4f, moment+update %.4f)   '
          'torch %8.4f [%8.4f, %8.4f]' % (
              (n, B) + step_ms + (inv_ms[0], code_ms[0], upd_ms[0]) +
              torch_ms))
    sys.stdout.flush()


if __name__ == '__main__':
  main()
