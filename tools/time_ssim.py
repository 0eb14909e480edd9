"""Times vtc_ssim (include/vtc_quality.h, csrc/ssim.hip) on float32 pairs of
512 x 512 and 2048 x 2048 and on a stack of 64 images of 256 x 256, with and
without the map:

  vtc_ssim              HIP-event median of the raw C call (both launches)
  compute_ssim_images   wall clock of the Python call with the ranges given,
                        ended by a device synchronise
  numpy restatement     wall clock of tests/ssim_oracle.py on the host of the
                        same box, for scale (one pass; the first image of the
                        stack, scaled to the whole stack)

The bytes a call must move are both inputs once, and the map once when it is
asked for; the rate printed is those bytes over the event time.  Every device
mean is checked against the restatement to 1e-9.

  timeout 900 python3 tools/time_ssim.py > profiles/ssim.txt
"""
import pathlib
import sys
import time

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'vision-transform-codes_amd'))
sys.path.insert(0, str(REPO / 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ssim_oracle  # noqa: E402
import vtc_hip  # noqa: E402
from utils import plotting  # noqa: E402

dev = torch.device('cuda:0')
WARMUP, REPS = 5, 50


def device_ms(fn):
  for _ in range(WARMUP):
    fn()
  times = []
  for _ in range(REPS):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    times.append(a.elapsed_time(b))
  return float(np.median(times)), float(np.min(times)), float(np.max(times))


def wall_ms(fn):
  for _ in range(WARMUP):
    fn()
  times = []
  for _ in range(REPS):
    torch.cuda.synchronize(dev)
    start = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    times.append((time.perf_counter() - start) * 1e3)
  return float(np.median(times))


def run(count, h, w):
  lib = vtc_hip.load_library()
  stream = vtc_hip.current_stream(dev)
  p = vtc_hip.ptr
  rs = np.random.RandomState(count + h + w)
  x = rs.rand(count, h, w).astype(np.float32)
  y = np.clip(x + 0.1 * rs.randn(count, h, w), 0., 1.).astype(np.float32)
  xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
  ranges = torch.ones(count, dtype=torch.float64, device=dev)
  means = torch.empty(count, dtype=torch.float64, device=dev)
  maps = torch.empty((count, h, w), dtype=torch.float64, device=dev)
  ws = vtc_hip.workspace(lib.vtc_ssim_workspace_bytes(count, h, w), dev)

  def raw(with_map):
    def call():
      vtc_hip.check(lib.vtc_ssim(
          p(xd), p(yd), vtc_hip.DTYPE_F32, p(ranges), p(means),
          p(maps if with_map else None), count, h, w, p(ws), ws.numel(),
          stream), 'vtc_ssim')
    return call

  start = time.perf_counter()
  want, want_map = ssim_oracle.ssim(x[0], y[0], 1.0)
  host_ms = (time.perf_counter() - start) * 1e3 * count

  print('%d x %d x %d float32, %d blocks' % (
      count, h, w, count * -(-h // 16) * -(-w // 32)))
  for with_map in (False, True):
    med, low, high = device_ms(raw(with_map))
    assert abs(float(means[0]) - want) <= 1e-9
    if with_map:
      assert float((maps[0].cpu() - torch.from_numpy(want_map)).abs().max()
                   ) <= 1e-9
    nbytes = count * h * w * (8 + (8 if with_map else 0))
    print('  %-34s %9.4f ms (min %.4f max %.4f)  %8.2f ns per sample  '
          '%7.1f GB/s' % ('vtc_ssim, ' + ('mean and map' if with_map
                                          else 'mean only'),
                          med, low, high, 1e6 * med / (count * h * w),
                          nbytes / (med * 1e-3) / 1e9))
  py = wall_ms(lambda: plotting.compute_ssim_images(xd, yd, ranges))
  print('  %-34s %9.4f ms' % ('compute_ssim_images (Python)', py))
  print('  %-34s %9.1f ms' % ('numpy restatement on the host', host_ms))


def main():
  print('device: %s' % torch.cuda.get_device_name(dev))
  print('command: timeout 900 python3 tools/time_ssim.py')
  print('HIP-event medians of %d after %d warm-up calls (raw C calls), '
        'wall-clock medians of %d (Python), one pass (host)'
        % (REPS, WARMUP, REPS))
  for count, h, w in ((1, 512, 512), (1, 2048, 2048), (64, 256, 256)):
    run(count, h, w)


if __name__ == '__main__':
  main()
