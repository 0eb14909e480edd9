"""Times vtc_index_code_unpack (include/vtc_index_decode.h) at the size of
tools/time_index_code.py -- the experiment's 100 000 patches, 41 scalar
columns of 64 codewords and the vector column of 4 096, 90 % zeros -- and on
the vector column alone (m = 1), to be read beside vtc_index_code_pack in
profiles/index_code.txt:

  vtc_index_code_unpack  HIP-event median of the raw C call: table
                         preparation, the decoding kernel, status
  tables                 the same call on the first row only: the status
                         kernels, the table preparation of all m columns and
                         one block of decoding
  decode                 the difference of the two
  unpack_index_streams   wall clock of the Python call: prefix check on the
                         host, table upload, workspace, the one host read
  host decoder           wall clock of a plain-Python decoder (a dictionary
                         lookup per candidate length) over the first 2 000
                         rows, for scale

The decoded indices are compared with the packed ones, all of them.  No
threshold: the numbers are a record.

  timeout 600 python3 tools/time_index_decode.py > profiles/index_decode.txt
"""
import pathlib
import sys
import time

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'vision-transform-codes_amd'))
sys.path.insert(0, str(REPO / 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vtc_hip  # noqa: E402
from utils import index_coding  # noqa: E402
from utils import jpeg  # noqa: E402
import time_index_code as packer  # noqa: E402  (the same indices and tables)

B, SAMPLE = packer.B, packer.SAMPLE
dev = packer.dev


def host_decode(bits, tables):
  """One row: the list of indices its string of '0' / '1' spells."""
  out, pos = [], 0
  for lookup in tables:
    for length, words in lookup:
      hit = words.get(bits[pos:pos + length])
      if hit is not None and pos + length <= len(bits):
        out.append(hit)
        pos += length
        break
    else:
      raise ValueError('no codeword')
  return out


def run(name, ks):
  lib = vtc_hip.load_library()
  stream = vtc_hip.current_stream(dev)
  p = vtc_hip.ptr
  rs = np.random.RandomState(len(ks))
  host = np.stack([packer.column(rs, k) for k in ks], axis=1)
  m, kmax = len(ks), max(ks)
  counts = np.stack([np.bincount(host[:, j], minlength=kmax)
                     for j in range(m)])
  tables = index_coding.index_huffman_tables(counts, ks)
  indices = torch.from_numpy(host).to(dev)
  t = index_coding._DeviceTables(tables, m, dev)
  packed, offsets = index_coding.pack_index_streams(indices, tables)
  total = int(offsets[-1])
  need = lib.vtc_index_code_unpack_workspace_bytes(m, kmax)
  print('%s: %d rows x %d columns, kmax %d, %d bits, %.2f MiB packed, '
        'workspace %.1f KiB, longest codeword %d bits'
        % (name, B, m, kmax, total, packed.numel() / 2.0 ** 20, need / 1024.0,
           max(len(w) for table in tables for w in table.values())))

  out = torch.empty((B, m), dtype=torch.int32, device=dev)
  rows = torch.empty(B, dtype=torch.int32, device=dev)
  status = torch.empty(3, dtype=torch.int64, device=dev)
  ws = vtc_hip.workspace(need, dev)

  def unpack(b):
    vtc_hip.check(lib.vtc_index_code_unpack(
        p(packed), packed.numel(), p(offsets), b, m, p(t.code), p(t.len), kmax,
        p(out), p(rows), p(status), p(ws), ws.numel(), stream),
                  'vtc_index_code_unpack')
  ms_tables = packer.device_ms(lambda: unpack(1))
  ms_all = packer.device_ms(lambda: unpack(B))
  assert status.tolist() == [0, 0, 0] and torch.equal(out, indices)
  assert int(rows.sum()) == total

  ms_py = packer.wall_ms(lambda: index_coding.unpack_index_streams(
      packed, offsets, tables))
  assert torch.equal(index_coding.unpack_index_streams(packed, offsets,
                                                       tables), indices)

  strings = [jpeg.stream_as_str(packed, offsets, r) for r in range(SAMPLE)]
  lookups = []
  for table in tables:
    words = {}
    for i, word in table.items():
      words.setdefault(len(word), {})[word] = i
    lookups.append(sorted(words.items()))
  start = time.perf_counter()
  decoded = [host_decode(bits, lookups) for bits in strings]
  ms_host = (time.perf_counter() - start) * 1e3
  assert decoded == host[:SAMPLE].tolist()

  for label, ms, rows_done in (
      ('vtc_index_code_unpack (raw C call)', ms_all, B),
      ('  tables (the call on one row)', ms_tables, B),
      ('  decode (the difference)', ms_all - ms_tables, B),
      ('unpack_index_streams (Python, all of it)', ms_py, B),
      ('host decoder, plain Python', ms_host, SAMPLE)):
    print('  %-42s %10.3f ms for %6d rows  %10.2f ns per row'
          % (label, ms, rows_done, 1e6 * ms / rows_done))


def main():
  print('device: %s' % torch.cuda.get_device_name(dev))
  print('command: timeout 600 python3 tools/time_index_decode.py')
  print('HIP-event medians of 20 (raw C calls), wall-clock medians of 5 '
        '(Python), one pass (host decoder)')
  run('experiment', [packer.SCALAR_K] * packer.SCALAR_COLUMNS +
      [packer.VECTOR_K])
  run('vector column alone', [packer.VECTOR_K])


if __name__ == '__main__':
  main()
