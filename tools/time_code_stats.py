"""Times the code statistics of include/vtc_stats.h (csrc/code_stats.hip) on
sparse float32 codes of 131 072 x 1024 and 1 048 576 x 64, about 70 % exact
zeros, with ignore = [0.0]:

  vtc_code_summary          HIP-event median of the raw C call (four launches,
                            the codes read twice)
  vtc_code_histogram        the same, 100 bins, the summary's ranges (two
                            launches, the codes read once)
  vtc_code_joint_histogram  64 pairs at 32 bins (four launches; every pair
                            reads its two columns twice)
  code_marginal_densities   wall clock of the Python call, its one host read
                            included
  copy                      HIP-event median of a device copy of the codes
                            (read + write), the HBM copy rate of this box and
                            this shape
  host route                the reference's way on the host of the same box:
                            the copy of the codes to the host, then per column
                            the filter, min, max, np.linspace, np.histogram
                            and np.var; timed on the first 32 columns and
                            scaled to all of them

The summary and the histogram should be read-bound; the fraction printed is
(bytes of codes read) / time over the measured copy rate (copy bytes = twice
the matrix).  The 1 048 576 x 64 matrix is exactly 256 MiB, the size of the
MI355X's last-level cache: repeated passes over it may be served partly from
that cache, the copy and the kernels alike, so its rates are not HBM rates; the
512 MiB matrix exceeds the cache.  The output says so.  The first eight
columns of every device result are checked against numpy.

  timeout 1100 python3 tools/time_code_stats.py > profiles/code_stats.txt
"""
import pathlib
import sys
import time

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'vision-transform-codes_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vtc_hip  # noqa: E402
from utils import plotting  # noqa: E402

dev = torch.device('cuda:0')
WARMUP, REPS = 5, 50
BINS, JOINT_PAIRS, JOINT_BINS, HOST_COLUMNS = 100, 64, 32, 32


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


def sparse_codes(b, s):
  """Laplacian codes with about 70 % exact zeros, made on the device."""
  gen = torch.Generator(device=dev)
  gen.manual_seed(b + s)
  u = torch.rand((b, s), device=dev, generator=gen) - 0.5
  # |u| = 0.5 would give log(0)
  codes = -torch.sign(u) * torch.log1p(-2 * u.abs().clamp(max=0.4999999))
  codes[torch.rand((b, s), device=dev, generator=gen) < 0.7] = 0.0
  return codes.contiguous()


def host_column(column, bins):
  kept = column[column != 0.0]
  edges = np.linspace(np.float64(kept.min()), np.float64(kept.max()), bins + 1)
  return np.histogram(kept.astype(np.float64), edges)[0], np.var(kept), kept


def run(b, s):
  lib = vtc_hip.load_library()
  stream = vtc_hip.current_stream(dev)
  p = vtc_hip.ptr
  codes = sparse_codes(b, s)
  nbytes = 4 * b * s
  ignore = torch.zeros(1, dtype=torch.float32, device=dev)
  kept, nonfinite = (torch.empty(s, dtype=torch.int64, device=dev)
                     for _ in range(2))
  lo, hi, mean, var = (torch.empty(s, dtype=torch.float64, device=dev)
                       for _ in range(4))
  counts = torch.empty((s, BINS), dtype=torch.int64, device=dev)
  ws_summary = vtc_hip.workspace(lib.vtc_code_summary_workspace_bytes(b, s),
                                 dev)
  ws_hist = vtc_hip.workspace(
      lib.vtc_code_histogram_workspace_bytes(b, s, BINS), dev)
  rs = np.random.RandomState(s)
  pairs = torch.from_numpy(
      rs.randint(0, s, size=(JOINT_PAIRS, 2)).astype(np.int32)).to(dev)
  jkept = torch.empty(JOINT_PAIRS, dtype=torch.int64, device=dev)
  jlo, jhi = (torch.empty((JOINT_PAIRS, 2), dtype=torch.float64, device=dev)
              for _ in range(2))
  jcounts = torch.empty((JOINT_PAIRS, JOINT_BINS, JOINT_BINS),
                        dtype=torch.int64, device=dev)
  ws_joint = vtc_hip.workspace(
      lib.vtc_code_joint_histogram_workspace_bytes(b, JOINT_PAIRS), dev)

  def summary():
    vtc_hip.check(lib.vtc_code_summary(
        p(codes), b, s, p(ignore), 1, p(kept), p(lo), p(hi), p(mean), p(var),
        p(nonfinite), p(ws_summary), ws_summary.numel(), stream),
                  'vtc_code_summary')

  def histogram():
    vtc_hip.check(lib.vtc_code_histogram(
        p(codes), b, s, p(ignore), 1, p(lo), p(hi), BINS, p(counts),
        p(ws_hist), ws_hist.numel(), stream), 'vtc_code_histogram')

  def joint():
    vtc_hip.check(lib.vtc_code_joint_histogram(
        p(codes), b, s, p(pairs), JOINT_PAIRS, s, p(ignore), 1, JOINT_BINS,
        p(jkept), p(jlo), p(jhi), p(jcounts), p(ws_joint), ws_joint.numel(),
        stream), 'vtc_code_joint_histogram')

  print('%d x %d float32 codes, %.0f MiB, %.1f %% zeros'
        % (b, s, nbytes / 2**20, 100 * float((codes == 0).float().mean())))
  if nbytes <= 256 << 20:
    print('  (no larger than the 256 MiB last-level cache: repeated passes may '
          'be served partly from it, so these are not HBM rates)')
  target = torch.empty_like(codes)
  copy_ms = device_ms(lambda: target.copy_(codes))[0]
  del target
  copy_rate = 2 * nbytes / (copy_ms * 1e-3)
  print('  %-36s %9.3f ms  %7.1f GB/s (read + write)'
        % ('device copy of the codes', copy_ms, copy_rate / 1e9))
  for name, fn, reads in (('vtc_code_summary', summary, 2),
                          ('vtc_code_histogram, %d bins' % BINS, histogram,
                           1)):
    med, low, high = device_ms(fn)
    rate = reads * nbytes / (med * 1e-3)
    print('  %-36s %9.3f ms (min %.3f max %.3f)  %7.1f GB/s read, %4.1f %% '
          'of the copy rate' % (name, med, low, high, rate / 1e9,
                                100 * rate / copy_rate))
  med, low, high = device_ms(joint)
  print('  %-36s %9.3f ms (min %.3f max %.3f)'
        % ('vtc_code_joint_histogram, %d pairs, %d bins'
           % (JOINT_PAIRS, JOINT_BINS), med, low, high))
  torch.cuda.synchronize(dev)
  start = time.perf_counter()
  plotting.code_marginal_densities(codes, BINS, [0.0])
  torch.cuda.synchronize(dev)
  print('  %-36s %9.3f ms (one call, its host read included)'
        % ('code_marginal_densities (Python)',
           (time.perf_counter() - start) * 1e3))

  # the host route, and the check of the device results against it
  start = time.perf_counter()
  on_host = codes.cpu().numpy()
  copy_s = time.perf_counter() - start
  start = time.perf_counter()
  columns = [host_column(on_host[:, c], BINS)
             for c in range(min(HOST_COLUMNS, s))]
  loop_s = (time.perf_counter() - start) * s / len(columns)
  for c in range(8):
    want_counts, _, values = columns[c]
    assert np.array_equal(counts[c].cpu().numpy(), want_counts), c
    assert int(kept[c]) == len(values)
    truth = np.var(values.astype(np.float64))
    assert abs(float(var[c]) - truth) <= 1e-9 * truth
  print('  %-36s %9.1f ms copy to the host + %.1f ms numpy loop over %d '
        'columns (timed on %d) = %.1f ms'
        % ('host route', copy_s * 1e3, loop_s * 1e3, s, len(columns),
           (copy_s + loop_s) * 1e3))


def main():
  print('device: %s' % torch.cuda.get_device_name(dev))
  print('command: timeout 1100 python3 tools/time_code_stats.py')
  print('HIP-event medians of %d after %d warm-up calls (raw C calls); the '
        'host route in one pass' % (REPS, WARMUP))
  for b, s in ((131072, 1024), (1048576, 64)):
    run(b, s)
    torch.cuda.empty_cache()


if __name__ == '__main__':
  main()
