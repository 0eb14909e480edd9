"""Times the four phases of ZCA whitening on one device with HIP events
(median of repeated runs): float64 covariance (centred), Jacobi
eigen-decomposition, forming W and W^-1, and the row transform y = (x - mu) W
+ m.  D = 2^20 rows of range-standardised-like data by default.

  python3 tools/time_zca.py [rows] [n ...]  > profiles/zca_whitening.txt
"""
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent /
                       'vision-transform-codes_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vtc_hip import linalg  # noqa: E402

dev = torch.device('cuda:0')


def median_ms(fn, reps):
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
  return float(np.median(times))


def main():
  rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
  sizes = [int(v) for v in sys.argv[2:]] or [64, 192, 256]
  print('device: %s' % torch.cuda.get_device_name(dev))
  print('rows D = %d; HIP-event medians' % rows)
  for n in sizes:
    g = torch.Generator(device=dev).manual_seed(n)
    x = 0.5 + 0.1 * torch.randn(rows, n, device=dev, generator=g)
    cov_ms = median_ms(lambda: linalg.column_covariance(x, True), 10)
    cov, means, grand = linalg.column_covariance(x, True)
    eig_ms = median_ms(lambda: linalg.sym_eig(cov), 3)
    w, u, status = linalg.sym_eig(cov)
    conv, sweeps = status.tolist()
    mat_ms = median_ms(lambda: linalg.zca_matrices(u, w), 10)
    wm, _ = linalg.zca_matrices(u, w)
    off = means.to(torch.float32)
    tr_ms = median_ms(lambda: linalg.row_transform(x, off, wm, 0.5), 10)
    gflop = 2.0 * rows * n * n / 1e9
    mib = 2.0 * rows * n * 4 / 2**20
    print('n = %3d  covariance %8.3f ms (%5.1f TFLOP/s f64)  '
          'eigen %8.3f ms (%d sweeps, converged %d)  matrices %7.3f ms  '
          'transform %8.3f ms (%6.1f GB/s, %5.1f TFLOP/s f32)' % (
              n, cov_ms, gflop / cov_ms, eig_ms, sweeps, conv, mat_ms,
              tr_ms, mib * 2**20 / tr_ms / 1e6, gflop / tr_ms))
    sys.stdout.flush()


if __name__ == '__main__':
  main()
