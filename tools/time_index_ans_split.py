"""Times the three calls of include/ext/vtc_index_ans_split.h on one column of
100 000 indices (half of them the zero codeword, a Zipf tail over the rest:
tests/index_ans_split_data.sparse_indices), with tables trained on the indices
themselves:

  kmax 4096     beside vtc_index_ans_sizes / _pack / _unpack of the same
                commit on the same indices in the same run (m = 1)
  kmax 131072   100 000 codewords in use, where only the split coder applies

HIP-event medians of 20 raw C calls each, at the default 65536 rows per stream
(two streams: two waves) and at 1024 rows per stream (98 streams).  Beside the
times: bits per index of the bytes, the empirical entropy, and the ideal cost
sum log2(2^15 / f) of the frequencies.  The device's streams are compared byte
for byte with the restatement of tests/index_ans_split_data.py and read back by
the decoder.  No threshold: the numbers are a record.

  timeout 600 python3 tools/time_index_ans_split.py \\
      > profiles/index_ans_split.txt
"""
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'vision-transform-codes_amd'))
sys.path.insert(0, str(REPO / 'tests'))
sys.path.insert(0, str(REPO / 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vtc_hip  # noqa: E402
from utils import index_coding  # noqa: E402
import index_ans_data as one_table  # noqa: E402
import index_ans_split_data as truth  # noqa: E402
import time_index_code as packer  # noqa: E402  (the timer)

B, dev, device_ms = packer.B, packer.dev, packer.device_ms
ROWS = (None, 1024)


def report(rows):
  for label, ms in rows:
    print('  %-44s %10.3f ms for %6d rows  %10.2f ns per row'
          % (label, ms, B, 1e6 * ms / B))


def split(lib, indices, host, tables, kmax, rows_per_stream):
  p, stream = vtc_hip.ptr, vtc_hip.current_stream(dev)
  packed, offsets, rows = index_coding.pack_index_ans_split(
      indices, tables, rows_per_stream)
  n, total = offsets.shape[0] - 1, packed.numel()
  streams, status = truth.encode(host, *tables, kmax, rows)
  assert status == [0, 0, 0]
  assert packed.cpu().numpy().tobytes() == b''.join(streams)
  back = index_coding.unpack_index_ans_split(packed, offsets, tables, B, rows)
  assert np.array_equal(back.cpu().numpy(), host)

  freq_hi = torch.from_numpy(tables[0].view(np.int16)).to(dev)
  freq_lo = torch.from_numpy(tables[1].view(np.int16)).to(dev)
  ws = vtc_hip.workspace(lib.vtc_index_ans_split_workspace_bytes(kmax), dev)
  sizes = torch.empty(n, dtype=torch.int32, device=dev)
  status = torch.empty(3, dtype=torch.int64, device=dev)
  ms_sizes = device_ms(lambda: vtc_hip.check(lib.vtc_index_ans_split_sizes(
      p(indices), B, p(freq_hi), p(freq_lo), kmax, rows, p(sizes), p(status),
      p(ws), ws.numel(), stream), 'vtc_index_ans_split_sizes'))
  assert status.tolist() == [0, 0, 0] and int(sizes.sum()) == total
  out = torch.empty_like(packed)
  ms_pack = device_ms(lambda: vtc_hip.check(lib.vtc_index_ans_split_pack(
      p(indices), B, p(freq_hi), p(freq_lo), kmax, rows, p(sizes), p(offsets),
      p(out), total, p(status), p(ws), ws.numel(), stream),
      'vtc_index_ans_split_pack'))
  assert status.tolist() == [0, 0, 0] and torch.equal(out, packed)
  got = torch.empty(B, dtype=torch.int32, device=dev)
  used = torch.empty(n, dtype=torch.int32, device=dev)
  ms_unpack = device_ms(lambda: vtc_hip.check(lib.vtc_index_ans_split_unpack(
      p(packed), total, p(offsets), B, p(freq_hi), p(freq_lo), kmax, rows,
      p(got), p(used), p(status), p(ws), ws.numel(), stream),
      'vtc_index_ans_split_unpack'))
  assert status.tolist() == [0, 0, 0] and torch.equal(got, indices)
  print('split coder, rows_per_stream %d: %d streams (waves), %d bytes = %.4f '
        'bits per index' % (rows, n, total, 8.0 * total / B))
  report((('vtc_index_ans_split_sizes', ms_sizes),
          ('vtc_index_ans_split_pack (zero-fill included)', ms_pack),
          ('vtc_index_ans_split_unpack', ms_unpack)))


def single(lib, indices, host, freq, rows_per_stream):
  """The one-table coder of include/vtc_index_ans.h on the same column."""
  p, stream = vtc_hip.ptr, vtc_hip.current_stream(dev)
  kmax = freq.shape[1]
  rows = index_coding.ANS_SPLIT_ROWS if rows_per_stream is None else (
      rows_per_stream)
  packed, offsets, rows = index_coding.pack_index_ans(indices, freq, rows)
  n, total = offsets.shape[0] - 1, packed.numel()
  device_freq = torch.from_numpy(freq.view(np.int16)).to(dev)
  ws = vtc_hip.workspace(lib.vtc_index_ans_workspace_bytes(1, kmax), dev)
  sizes = torch.empty(n, dtype=torch.int32, device=dev)
  status = torch.empty(3, dtype=torch.int64, device=dev)
  ms_sizes = device_ms(lambda: vtc_hip.check(lib.vtc_index_ans_sizes(
      p(indices), B, 1, p(device_freq), kmax, rows, p(sizes), p(status), p(ws),
      ws.numel(), stream), 'vtc_index_ans_sizes'))
  out = torch.empty_like(packed)
  ms_pack = device_ms(lambda: vtc_hip.check(lib.vtc_index_ans_pack(
      p(indices), B, 1, p(device_freq), kmax, rows, p(sizes), p(offsets),
      p(out), total, p(status), p(ws), ws.numel(), stream),
      'vtc_index_ans_pack'))
  assert torch.equal(out, packed)
  got = torch.empty((B, 1), dtype=torch.int32, device=dev)
  used = torch.empty(n, dtype=torch.int32, device=dev)
  ms_unpack = device_ms(lambda: vtc_hip.check(lib.vtc_index_ans_unpack(
      p(packed), total, p(offsets), B, 1, p(device_freq), kmax, rows, p(got),
      p(used), p(status), p(ws), ws.numel(), stream), 'vtc_index_ans_unpack'))
  assert status.tolist() == [0, 0, 0] and torch.equal(got[:, 0], indices)
  print('one-table coder, rows_per_stream %d: %d streams, %d bytes = %.4f bits '
        'per index; ideal cost %.4f'
        % (rows, n, total, 8.0 * total / B,
           one_table.ideal_bits(host[:, None], freq) / B))
  report((('vtc_index_ans_sizes', ms_sizes),
          ('vtc_index_ans_pack (zero-fill included)', ms_pack),
          ('vtc_index_ans_unpack', ms_unpack)))


def main():
  lib = vtc_hip.load_library()
  print('device: %s' % torch.cuda.get_device_name(dev))
  print('command: timeout 600 python3 tools/time_index_ans_split.py')
  print('measured: every time below is a HIP-event median of 20 raw C calls; '
        'every bit count is of bytes the decoder read back')
  for kmax, k in ((4096, 4096), (131072, 100000)):
    host = truth.sparse_indices(kmax, B, k, 0.5)
    counts = np.bincount(host, minlength=kmax)
    indices = torch.from_numpy(host).to(dev)
    tables = index_coding.index_ans_split_frequencies(counts, k)
    want = truth.frequencies(counts.tolist(), k)
    assert all(np.array_equal(a, b) for a, b in zip(tables, want))
    print('kmax %d, %d codewords in use, %d rows, %.1f %% zeros, %d distinct '
          'indices; empirical entropy %.4f bits per index, ideal cost under '
          'the two 15-bit tables %.4f'
          % (kmax, k, B, 100.0 * float((host == 0).mean()),
             int((counts > 0).sum()), truth.entropy_bits(host, kmax) / B,
             truth.ideal_bits(host, *tables) / B))
    for rows_per_stream in ROWS:
      split(lib, indices, host, tables, kmax, rows_per_stream)
      if kmax <= index_coding.MAX_SYMBOLS:
        single(lib, indices, host,
               index_coding.index_ans_frequencies(counts[None, :], [k]),
               rows_per_stream)


if __name__ == '__main__':
  main()
