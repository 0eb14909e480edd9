"""Times the baseline JFIF reader of include/ext/vtc_jfif_decode.h on one
device: the seeded 768 x 512 colour image of tools/time_jfif.py at 4:2:0,
quality 75 and quality 95, written by utils.jfif.encode_rgb.  Each raw C call
of the chain on preallocated arrays (HIP-event medians of windows of 20 calls,
after warm-up), the synchronisation rounds the unpack took,
utils.jfif.decode_bytes end to end (host marker walk, upload and the one
status read included, wall clock around a synchronise), and PIL's decoder on
one host thread of the same box for scale.  Then the input that never
synchronises -- 768 x 512 gray noise at quality 100 -- whose unpack costs what a
sequential walk costs.

  python3 tools/time_jfif_decode.py > profiles/jfif_decode.txt
"""
import io
import pathlib
import sys
import time

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent /
                       'vision-transform-codes_amd'))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vtc_hip  # noqa: E402
from utils import jfif  # noqa: E402
import time_jfif  # noqa: E402

dev = time_jfif.dev
H, W = time_jfif.H, time_jfif.W
report = time_jfif.report


def chain(lib, stream, data):
  up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
  headers = jfif.parse_headers(data)
  layout = jfif.frame_layout(headers['shape'], headers['sampling'])
  at = headers['segment_at']
  stuffed = up(np.frombuffer(data, dtype=np.uint8, offset=at).copy())
  n = stuffed.numel()
  out = torch.empty(n, dtype=torch.uint8, device=dev)
  meta = torch.zeros(8, dtype=torch.int64, device=dev)
  ws = vtc_hip.workspace(lib.vtc_jfif_unstuff_bytes_workspace_bytes(n), dev)
  total = 0.

  def unstuff():
    vtc_hip.check(lib.vtc_jfif_unstuff_bytes(
        vtc_hip.ptr(stuffed), n, vtc_hip.ptr(out), n, vtc_hip.ptr(meta),
        vtc_hip.ptr(meta[2:3]), vtc_hip.ptr(ws), ws.numel(), stream),
                  'vtc_jfif_unstuff_bytes')
  unstuff()
  seg_bytes, marker_at = (int(v) for v in meta[:2].cpu())
  total += report('vtc_jfif_unstuff_bytes, %d bytes, %d zeros removed'
                  % (n, marker_at - seg_bytes), unstuff)

  d = layout['rows']
  tables = jfif._DecodeTables(headers['tables'], dev)
  slot_dc, slot_ac = jfif._slots(layout, headers['selectors'])
  nslots = len(slot_dc)
  slot_dc, slot_ac = up(slot_dc), up(slot_ac)
  levels = torch.empty((d, 64), dtype=torch.int32, device=dev)
  ws2 = vtc_hip.workspace(lib.vtc_jfif_unpack_workspace_bytes(seg_bytes), dev)

  def unpack():
    vtc_hip.check(lib.vtc_jfif_unpack(
        vtc_hip.ptr(out), seg_bytes, vtc_hip.ptr(slot_dc), vtc_hip.ptr(slot_ac),
        nslots, vtc_hip.ptr(tables.ac_code), vtc_hip.ptr(tables.ac_len),
        vtc_hip.ptr(tables.dc_code), vtc_hip.ptr(tables.dc_len),
        vtc_hip.ptr(levels), d, vtc_hip.ptr(meta[4:8]), vtc_hip.ptr(ws2),
        ws2.numel(), stream), 'vtc_jfif_unpack')
  unpack()
  status = meta[4:8].cpu().tolist()
  subsequences = -(-seg_bytes // vtc_hip.JFIF_SUBSEQ_BYTES)
  groups = -(-subsequences // vtc_hip.JFIF_SUBSEQ_PER_GROUP)
  total += report('vtc_jfif_unpack, %d bytes, %d blocks' % (seg_bytes, d),
                  unpack)
  print('    %d subsequences in %d workgroups (%d launches), %d '
        'synchronisation rounds, status %s' % (subsequences, groups, groups,
                                               status[3], status[:3]))

  order, start = up(layout['order']), up(layout['start'])
  ws3 = vtc_hip.workspace(lib.vtc_jfif_dc_accumulate_workspace_bytes(d), dev)

  def accumulate():    # on DIFFs or on sums: the same work
    vtc_hip.check(lib.vtc_jfif_dc_accumulate(
        vtc_hip.ptr(levels), d, vtc_hip.ptr(order), vtc_hip.ptr(start),
        vtc_hip.ptr(ws3), ws3.numel(), stream), 'vtc_jfif_dc_accumulate')
  total += report('vtc_jfif_dc_accumulate, %d blocks' % d, accumulate)

  basis = up(jfif.dct_basis())
  for c, comp in enumerate(headers['components']):
    q = up(headers['qtables'][comp[3]].view(np.int16))
    rob = up(layout['row_of_block'][c])
    h, w = layout['plane_shapes'][c]
    bh, bw = layout['grids'][c]
    plane = torch.empty((h, w), dtype=torch.float32, device=dev)

    def inverse():
      vtc_hip.check(lib.vtc_jfif_inverse_dct(
          vtc_hip.ptr(levels), d, vtc_hip.ptr(rob), bh, bw,
          vtc_hip.ptr(basis), vtc_hip.ptr(q), vtc_hip.ptr(plane), h, w,
          stream), 'vtc_jfif_inverse_dct')
    name = 'Y Cb Cr'.split()[c] if len(headers['components']) == 3 else 'Y'
    total += report('vtc_jfif_inverse_dct %s %d x %d' % (name, h, w), inverse)
  print('  %-46s %8.4f ms' % ('sum of the device calls', total))


def end_to_end(data):
  times = []
  for _ in range(8):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    image, info = jfif.decode_bytes(data)
    torch.cuda.synchronize(dev)
    times.append((time.perf_counter() - t0) * 1e3)
  print('  %-46s %8.3f ms (median of the last 5 of 8, wall clock)'
        % ('utils.jfif.decode_bytes end to end', np.median(times[3:])))
  return image


def pil_decoder(data, ours):
  try:
    from PIL import Image
  except ImportError:
    print('  PIL is not installed: no host decoder for scale')
    return
  times = []
  for _ in range(8):
    t0 = time.perf_counter()
    picture = Image.open(io.BytesIO(data))
    picture.load()
    times.append((time.perf_counter() - t0) * 1e3)
  print('  %-46s %8.3f ms (median of the last 5 of 8, wall clock, one host '
        'thread)' % ('PIL open + load on the host', np.median(times[3:])))
  theirs = np.asarray(picture).astype(np.float64)
  worst = np.abs(theirs - ours.cpu().numpy()).max()
  print('  largest difference from PIL\'s picture: %g grey levels (its IDCT '
        'is an integer one and its chroma filter another)' % worst)


def main():
  lib = vtc_hip.load_library()
  stream = vtc_hip.current_stream(dev)
  host = time_jfif.picture()
  image = torch.from_numpy(host).to(dev)
  print('device: %s' % torch.cuda.get_device_name(dev))
  print('command: python3 tools/time_jfif_decode.py')
  print('%d x %d x 3 float32 image, YCbCr 4:2:0, written by '
        'utils.jfif.encode_rgb; HIP-event medians (min .. max) of %d windows '
        'of %d raw C calls after 3 warm-up calls'
        % (W, H, time_jfif.WINDOWS, time_jfif.CALLS))
  for quality in (75, 95):
    data, _ = jfif.encode_rgb(image, (2, 2), quality)
    print('quality %d: a file of %d bytes' % (quality, len(data)))
    chain(lib, stream, data)
    pil_decoder(data, end_to_end(data))
  noise = torch.from_numpy(np.random.RandomState(5).randint(
      0, 256, size=(H, W)).astype(np.float32)).to(dev)
  data, _ = jfif.encode_gray(noise, 100)
  print('%d x %d gray noise at quality 100 (63 nonzero coefficients a block: '
        'no end of block, the decode never synchronises): a file of %d bytes'
        % (W, H, len(data)))
  chain(lib, stream, data)
  pil_decoder(data, end_to_end(data))
  print('not measured: hardware counters, images above this size, files of '
        'other encoders.')


if __name__ == '__main__':
  main()
