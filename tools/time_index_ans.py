"""Times the three calls of include/vtc_index_ans.h at the experiment's size
(the indices of tools/time_index_code.py: 100 000 patches, 41 scalar columns
and the vector column, 90 % zeros in every column), beside the Huffman calls of
the same commit on the same indices, and reports the bytes of both codes:

  vtc_index_ans_sizes    HIP-event median of the raw C call: status, the
                         cumulative sums, the coder run without stores
  vtc_index_ans_pack     the same with the zero-fill of the output and stores
  vtc_index_ans_unpack   status, the cumulative sums, the decoder
  vtc_index_code_bits,
  vtc_index_code_pack    the Huffman calls, as tools/time_index_code.py times
                         them

at the default rows_per_stream (max(1, 65536 // m): few, long streams, one
wave each) and at 512 and 64 rows per stream (more and shorter ones, more
flush bytes), so a caller can see the trade.  The frequencies and the Huffman
tables are trained on the indices themselves.  Beside the bytes: the empirical
entropy, the ideal cost sum log2(2^15 / f) of the frequencies, and the coder's
excess over it, the 256-byte flush of every stream included.  The device's streams are
compared byte for byte with the restatement of tests/index_ans_data.py and
read back by the decoder.  No threshold: the numbers are a record.

  timeout 600 python3 tools/time_index_ans.py > profiles/index_ans.txt
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
import index_ans_data as truth  # noqa: E402
import time_index_code as packer  # noqa: E402  (the same indices)

B, dev, device_ms = packer.B, packer.dev, packer.device_ms
ROWS = (None, 512, 64)


def huffman(lib, indices, host, counts, ks):
  """(bits, ms of vtc_index_code_bits, ms of vtc_index_code_pack)."""
  p, stream = vtc_hip.ptr, vtc_hip.current_stream(dev)
  m, kmax = len(ks), max(ks)
  tables = index_coding.index_huffman_tables(counts, ks)
  t = index_coding._DeviceTables(tables, m, dev)
  packed, offsets = index_coding.pack_index_streams(indices, tables)
  rows = torch.empty(B, dtype=torch.int32, device=dev)
  cols = torch.empty(m, dtype=torch.int64, device=dev)
  status = torch.empty(3, dtype=torch.int64, device=dev)
  ms_bits = device_ms(lambda: vtc_hip.check(lib.vtc_index_code_bits(
      p(indices), B, m, p(t.len), kmax, p(rows), p(cols), p(status), stream),
      'vtc_index_code_bits'))
  out = torch.empty_like(packed)
  ms_pack = device_ms(lambda: vtc_hip.check(lib.vtc_index_code_pack(
      p(indices), B, m, p(t.code), p(t.len), kmax, p(offsets), p(out),
      out.numel(), p(status), stream), 'vtc_index_code_pack'))
  assert torch.equal(out, packed)
  return int(offsets[-1]), ms_bits, ms_pack


def ans(lib, indices, host, host_freq, rows_per_stream, ideal):
  p, stream = vtc_hip.ptr, vtc_hip.current_stream(dev)
  m, kmax = host_freq.shape
  packed, offsets, rows = index_coding.pack_index_ans(indices, host_freq,
                                                      rows_per_stream)
  n = offsets.shape[0] - 1
  total = packed.numel()
  streams, status = truth.encode(host, host_freq, rows)
  assert status == [0, 0, 0]
  assert packed.cpu().numpy().tobytes() == b''.join(streams)
  back = index_coding.unpack_index_ans(packed, offsets, host_freq, B, rows)
  assert np.array_equal(back.cpu().numpy(), host)

  freq = torch.from_numpy(host_freq.view(np.int16)).to(dev)
  ws = vtc_hip.workspace(lib.vtc_index_ans_workspace_bytes(m, kmax), dev)
  sizes = torch.empty(n, dtype=torch.int32, device=dev)
  status = torch.empty(3, dtype=torch.int64, device=dev)
  ms_sizes = device_ms(lambda: vtc_hip.check(lib.vtc_index_ans_sizes(
      p(indices), B, m, p(freq), kmax, rows, p(sizes), p(status), p(ws),
      ws.numel(), stream), 'vtc_index_ans_sizes'))
  assert status.tolist() == [0, 0, 0] and int(sizes.sum()) == total
  out = torch.empty_like(packed)
  ms_pack = device_ms(lambda: vtc_hip.check(lib.vtc_index_ans_pack(
      p(indices), B, m, p(freq), kmax, rows, p(sizes), p(offsets), p(out),
      total, p(status), p(ws), ws.numel(), stream), 'vtc_index_ans_pack'))
  assert status.tolist() == [0, 0, 0] and torch.equal(out, packed)
  got = torch.empty((B, m), dtype=torch.int32, device=dev)
  used = torch.empty(n, dtype=torch.int32, device=dev)
  ms_unpack = device_ms(lambda: vtc_hip.check(lib.vtc_index_ans_unpack(
      p(packed), total, p(offsets), B, m, p(freq), kmax, rows, p(got), p(used),
      p(status), p(ws), ws.numel(), stream), 'vtc_index_ans_unpack'))
  assert status.tolist() == [0, 0, 0] and torch.equal(got, indices)

  bits, flush = 8 * total, 8 * truth.HEADER * n
  per = float(B * m)
  print('rows_per_stream %d: %d streams (waves), %d bytes = %.4f bits per '
        'index, of which the end states %.4f; excess over the ideal cost '
        '%.4f %%'
        % (rows, n, total, bits / per, flush / per,
           100.0 * (bits - ideal) / ideal))
  for label, ms in (('vtc_index_ans_sizes', ms_sizes),
                    ('vtc_index_ans_pack (zero-fill included)', ms_pack),
                    ('vtc_index_ans_unpack', ms_unpack)):
    print('  %-42s %10.3f ms for %6d rows  %10.2f ns per row'
          % (label, ms, B, 1e6 * ms / B))
  return bits


def main():
  lib = vtc_hip.load_library()
  print('device: %s' % torch.cuda.get_device_name(dev))
  print('command: timeout 600 python3 tools/time_index_ans.py')
  print('HIP-event medians of 20 raw C calls')
  ks = [packer.SCALAR_K] * packer.SCALAR_COLUMNS + [packer.VECTOR_K]
  m, kmax = len(ks), max(ks)
  rs = np.random.RandomState(len(ks))
  host = np.stack([packer.column(rs, k) for k in ks], axis=1)
  counts = np.stack([np.bincount(host[:, j], minlength=kmax)
                     for j in range(m)])
  indices = torch.from_numpy(host).to(dev)
  host_freq = index_coding.index_ans_frequencies(counts, ks)
  assert np.array_equal(host_freq, truth.frequency_array(counts, ks))
  entropy = truth.entropy_bits(host, kmax)
  ideal = truth.ideal_bits(host, host_freq)
  per = float(B * m)
  print('experiment: %d rows x %d columns, kmax %d, %.1f %% zeros; empirical '
        'entropy %.4f bits per index, ideal cost under the 15-bit frequencies '
        '%.4f' % (B, m, kmax, 100.0 * float((host == 0).mean()), entropy / per,
                  ideal / per))
  huffman_bits, ms_bits, ms_pack = huffman(lib, indices, host, counts, ks)
  print('Huffman (index_huffman_tables): %d bytes = %.4f bits per index'
        % (-(-huffman_bits // 8), huffman_bits / per))
  for label, ms in (('vtc_index_code_bits', ms_bits),
                    ('vtc_index_code_pack (zero-fill included)', ms_pack)):
    print('  %-42s %10.3f ms for %6d rows  %10.2f ns per row'
          % (label, ms, B, 1e6 * ms / B))
  for rows_per_stream in ROWS:
    bits = ans(lib, indices, host, host_freq, rows_per_stream, ideal)
    print('  range coder / Huffman bytes: %.4f' % (bits / float(huffman_bits)))


if __name__ == '__main__':
  main()
