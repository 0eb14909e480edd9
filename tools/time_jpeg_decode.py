"""Times the decoder of include/vtc_decode.h beside the packer it inverts, on
131 072 patches of 64 and of 256 levels, quantised from Laplacian DCT-like
codes as in tools/time_jpeg.py (the Annex K.1 bin widths; for 256 levels the
widths beyond the 64th repeat the last one):

  vtc_jpeg_unpack   HIP-event median of the raw C call: zero-fill, tables,
                    decode
  unpack_streams    wall clock of the Python call, its status read included
  vtc_jpeg_pack     HIP-event median of the raw C call on the same levels
  host decoder      wall clock of a plain Python decoder (a dict of codewords,
                    one bit string per row) on the first 1 024 rows

Every decode is checked against the levels that were packed.

  timeout 600 python3 tools/time_jpeg_decode.py > profiles/jpeg_decoding.txt
"""
import pathlib
import sys
import time

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'vision-transform-codes_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vtc_hip  # noqa: E402
from utils import jpeg  # noqa: E402

D = 1 << 17
SAMPLE = 1024
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


def host_decode(bits, s, table_ac, table_dc):
  """One row from its string of '0' and '1' by the rules of DESIGN.md 4.12;
  the streams here are well formed."""
  ac = {word: jpeg._AC_BYTE[symbol] for symbol, word in table_ac.items()}
  dc = {word: jpeg._DC_CATEGORY[symbol] for symbol, word in table_dc.items()}

  def symbol(table, at):
    stop = at + 1
    while bits[at:stop] not in table:
      stop += 1
    return table[bits[at:stop]], stop

  def value(at, size):
    raw = int(bits[at:at + size], 2)
    return raw if bits[at] == '1' else raw - ((1 << size) - 1)

  row = np.zeros(s, dtype=np.int32)
  at, k = 0, 1
  while True:
    byte, at = symbol(ac, at)
    if byte == 0x00:
      break
    if byte == 0xF0:
      k += 16
      continue
    k += byte >> 4
    row[k] = value(at, byte & 15)
    at += byte & 15
    k += 1
  category, at = symbol(dc, at)
  if category:
    row[0] = value(at, category)
    at += category
  assert at == len(bits)
  return row


def levels_of(s):
  widths = jpeg.get_jpeg_quant_hifi_binwidths()
  widths = np.concatenate([widths, np.full(max(0, s - 64), widths[-1])])[:s]
  rs = np.random.RandomState(s)
  scale = 300.0 / (1.0 + np.arange(s)) ** 1.2
  levels = torch.empty((D, s), dtype=torch.int32, device=dev)
  step = 1 << 14
  for start in range(0, D, step):
    codes = (rs.laplace(size=(step, s)) * scale).astype(np.float32)
    levels[start:start + step] = jpeg.quantize(
        torch.from_numpy(codes).to(dev), widths)
  return levels


def run(s):
  lib = vtc_hip.load_library()
  stream = vtc_hip.current_stream(dev)
  p = vtc_hip.ptr
  levels = levels_of(s)
  tables = jpeg.tables_from_counts(*jpeg.symbol_counts(levels))
  t = jpeg._DeviceTables(tables[0], tables[1], dev)
  packed, offsets = jpeg.pack_streams(levels, *tables)
  total = int(offsets[-1])
  print('%d patches x %d levels: %.1f %% nonzero, %d bits = %.3f bits per '
        'level, %.2f MiB packed, longest codeword %d bits'
        % (D, s, 100.0 * float((levels != 0).float().mean()), total,
           total / float(D * s), packed.numel() / 2.0 ** 20,
           max(len(w) for w in list(tables[0].values()) +
               list(tables[1].values()))))

  back = torch.empty_like(levels)
  status = torch.empty(3, dtype=torch.int64, device=dev)
  ws = vtc_hip.workspace(lib.vtc_jpeg_unpack_workspace_bytes(), dev)

  def run_unpack():
    vtc_hip.check(lib.vtc_jpeg_unpack(
        p(packed), packed.numel(), p(offsets), D, s, p(t.ac_code),
        p(t.ac_len), p(t.dc_code), p(t.dc_len), p(back), p(status), p(ws),
        ws.numel(), stream), 'vtc_jpeg_unpack')
  ms_unpack = device_ms(run_unpack)
  assert status.tolist() == [0, 0, 0] and torch.equal(back, levels)

  ms_python = wall_ms(lambda: jpeg.unpack_streams(packed, offsets, s, *tables))
  assert torch.equal(jpeg.unpack_streams(packed, offsets, s, *tables), levels)

  out = torch.empty_like(packed)
  pack_status = torch.empty(2, dtype=torch.int32, device=dev)

  def run_pack():
    vtc_hip.check(lib.vtc_jpeg_pack(
        p(levels), D, s, p(t.ac_code), p(t.ac_len), p(t.dc_code), p(t.dc_len),
        p(offsets), p(out), out.numel(), p(pack_status), stream),
                  'vtc_jpeg_pack')
  ms_pack = device_ms(run_pack)
  assert pack_status.tolist() == [0, 0] and torch.equal(out, packed)

  strings = [jpeg.stream_as_str(packed, offsets, i) for i in range(SAMPLE)]
  start = time.perf_counter()
  rows = np.stack([host_decode(x, s, *tables) for x in strings])
  ms_host = (time.perf_counter() - start) * 1e3
  assert np.array_equal(rows, levels[:SAMPLE].cpu().numpy())

  for name, ms, rows_done in (
      ('vtc_jpeg_unpack (zero-fill included)', ms_unpack, D),
      ('unpack_streams (Python, status read)', ms_python, D),
      ('vtc_jpeg_pack (zero-fill included)', ms_pack, D),
      ('host decoder, plain Python', ms_host, SAMPLE)):
    print('  %-38s %10.3f ms for %6d rows  %10.2f ns per row  %8.3f Gbit/s '
          'of stream' % (name, ms, rows_done, 1e6 * ms / rows_done,
                         total * (rows_done / float(D)) / (ms * 1e-3) / 1e9))


def main():
  print('device: %s' % torch.cuda.get_device_name(dev))
  print('command: timeout 600 python3 tools/time_jpeg_decode.py')
  print('HIP-event medians of 20 (raw C calls), wall-clock medians of 5 '
        '(Python), one pass (host decoder)')
  for s in (64, 256):
    run(s)


if __name__ == '__main__':
  main()
