"""Times the two kernels of include/vtc_index_code.h at the experiment's size
(experiments/rate_distortion_sparse_coding.py: 100 000 patches, 41 scalar
columns and the vector column) and on the vector column alone (m = 1):

  vtc_index_code_bits   HIP-event median of the raw C call: status, zero-fill
                        of the column sums, the kernel
  vtc_index_code_pack   HIP-event median of the raw C call: zero-fill of the
                        output, the kernel
  index_code_bits,
  pack_index_streams    wall clock of the Python calls, table upload, offsets
                        and status reads included
  host join             wall clock of ''.join(table[j][i] ...) over the first
                        2 000 rows on the host, for scale

The indices are 90 % zeros in every column (index 0 is the zero codeword); the
rest are geometric over 64 scalar codewords and 4 096 vector codewords.  The
tables are trained on the indices themselves.  The packed streams are checked
against the host join on the sample.  No threshold: the numbers are a record.

  timeout 600 python3 tools/time_index_code.py > profiles/index_code.txt
"""
import pathlib
import sys
import time

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'vision-transform-codes_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vtc_hip  # noqa: E402
from utils import index_coding  # noqa: E402
from utils import jpeg  # noqa: E402

B = 100000
SAMPLE = 2000
SCALAR_COLUMNS, SCALAR_K, VECTOR_K = 41, 64, 4096
dev = torch.device('cuda:0')


def device_ms(fn, reps=20):
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


def wall_ms(fn, reps=5):
  fn()
  times = []
  for _ in range(reps):
    torch.cuda.synchronize(dev)
    start = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    times.append((time.perf_counter() - start) * 1e3)
  return float(np.median(times))


def column(rs, k):
  """90 % zeros, the rest geometric over 1 .. k - 1."""
  other = 1 + np.minimum(rs.geometric(16.0 / k, size=B) - 1, k - 2)
  return np.where(rs.rand(B) < 0.9, 0, other).astype(np.int32)


def run(name, ks):
  lib = vtc_hip.load_library()
  stream = vtc_hip.current_stream(dev)
  p = vtc_hip.ptr
  rs = np.random.RandomState(len(ks))
  host = np.stack([column(rs, k) for k in ks], axis=1)
  m, kmax = len(ks), max(ks)
  counts = np.stack([np.bincount(host[:, j], minlength=kmax)
                     for j in range(m)])
  tables = index_coding.index_huffman_tables(counts, ks)
  indices = torch.from_numpy(host).to(dev)
  t = index_coding._DeviceTables(tables, m, dev)
  assert t.kmax == kmax
  packed, offsets = index_coding.pack_index_streams(indices, tables)
  total = int(offsets[-1])
  print('%s: %d rows x %d columns, kmax %d, %.1f %% zeros, %d bits = %.3f '
        'bits per index, %.2f MiB packed, tables %.1f KiB, longest codeword '
        '%d bits'
        % (name, B, m, kmax, 100.0 * float((host == 0).mean()), total,
           total / float(B * m), packed.numel() / 2.0 ** 20,
           m * kmax * 9 / 1024.0,
           max(len(w) for table in tables for w in table.values())))

  rows = torch.empty(B, dtype=torch.int32, device=dev)
  cols = torch.empty(m, dtype=torch.int64, device=dev)
  status = torch.empty(3, dtype=torch.int64, device=dev)

  def run_bits():
    vtc_hip.check(lib.vtc_index_code_bits(
        p(indices), B, m, p(t.len), kmax, p(rows), p(cols), p(status),
        stream), 'vtc_index_code_bits')
  ms_bits = device_ms(run_bits)
  assert status.tolist() == [0, 0, 0] and int(cols.sum()) == total

  out = torch.empty_like(packed)

  def run_pack():
    vtc_hip.check(lib.vtc_index_code_pack(
        p(indices), B, m, p(t.code), p(t.len), kmax, p(offsets), p(out),
        out.numel(), p(status), stream), 'vtc_index_code_pack')
  ms_pack = device_ms(run_pack)
  assert status.tolist() == [0, 0, 0] and torch.equal(out, packed)

  ms_py_bits = wall_ms(lambda: index_coding.index_code_bits(indices, tables))
  ms_py_pack = wall_ms(lambda: index_coding.pack_index_streams(indices,
                                                               tables))

  start = time.perf_counter()
  strings = [''.join(tables[j][i] for j, i in enumerate(row))
             for row in host[:SAMPLE].tolist()]
  ms_host = (time.perf_counter() - start) * 1e3
  for r in range(0, SAMPLE, 97):
    assert jpeg.stream_as_str(packed, offsets, r) == strings[r]

  for label, ms, rows_done in (
      ('vtc_index_code_bits (raw C call)', ms_bits, B),
      ('vtc_index_code_pack (zero-fill included)', ms_pack, B),
      ('index_code_bits (Python, tables, status)', ms_py_bits, B),
      ('pack_index_streams (Python, all of it)', ms_py_pack, B),
      ('host join, plain Python', ms_host, SAMPLE)):
    print('  %-42s %10.3f ms for %6d rows  %10.2f ns per row'
          % (label, ms, rows_done, 1e6 * ms / rows_done))


def main():
  print('device: %s' % torch.cuda.get_device_name(dev))
  print('command: timeout 600 python3 tools/time_index_code.py')
  print('HIP-event medians of 20 (raw C calls), wall-clock medians of 5 '
        '(Python), one pass (host join)')
  run('experiment', [SCALAR_K] * SCALAR_COLUMNS + [VECTOR_K])
  run('vector column alone', [VECTOR_K])


if __name__ == '__main__':
  main()
