"""Builders for the tests of the baseline JFIF reader (utils/jfif.py,
include/ext/vtc_jfif_decode.h): the sequential decoder the device unpack must
equal, written from the header's text alone; the foreign files of
tests/golden/jfif_foreign.npz and how they were made; byte strings with one
header field changed; the three device-free restatements of the small calls.
numpy only."""
import io
import pathlib

import numpy as np

import jfif_data as truth

GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden' / 'jfif_foreign.npz'
SUBSEQ_BYTES = 128
GROUP_BYTES = 256 * SUBSEQ_BYTES

# name -> PIL's save arguments; the image is foreign_image()
FOREIGN = {
    'gray': dict(mode='L', quality=85, optimize=True),
    '444': dict(mode='RGB', quality=85, optimize=True, subsampling=0),
    '422': dict(mode='RGB', quality=85, optimize=True, subsampling=1),
    '420': dict(mode='RGB', quality=85, optimize=True, subsampling=2),
    '420-default-tables': dict(mode='RGB', quality=85, optimize=False,
                               subsampling=2),
}


def foreign_image():
  """uint8 (64, 96, 3): the seeded colour image of tests/color_data.py."""
  return np.rint(truth.colour_image(64, 96, seed=2024)).astype(np.uint8)


def make_foreign():
  """{name: uint8 bytes} written by PIL (needs PIL): what
  tests/golden/jfif_foreign.npz holds."""
  from PIL import Image
  out = {}
  rgb = foreign_image()
  for name, args in FOREIGN.items():
    args = dict(args)
    mode = args.pop('mode')
    picture = Image.fromarray(rgb)
    if mode == 'L':
      picture = picture.convert('L')
    buf = io.BytesIO()
    picture.save(buf, format='JPEG', **args)
    out[name] = np.frombuffer(buf.getvalue(), dtype=np.uint8).copy()
  return out


def load_foreign():
  with np.load(GOLDEN) as g:
    return {name: g[name].tobytes() for name in g.files}


# -------------------------------------------------------- the small calls
def unstuff(data):
  """(bytes, marker_at) as vtc_jfif_unstuff_bytes defines them."""
  data = bytes(data)
  marker_at = len(data)
  for i, b in enumerate(data):
    if b == 0xFF and (i + 1 >= len(data) or data[i + 1] != 0x00):
      marker_at = i
      break
  return data[:marker_at].replace(b'\xff\x00', b'\xff'), marker_at


def dc_accumulate(levels, order, start):
  """levels with column 0 accumulated along order, int32 wrapping."""
  out = np.array(levels, dtype=np.int32)
  d, acc = out.shape[0], 0
  for j in range(len(order)):
    if start[j]:
      acc = 0
    r = int(order[j])
    if 0 <= r < d:
      acc = (acc + int(out[r, 0])) & 0xFFFFFFFF
      out[r, 0] = acc - (1 << 32) if acc >> 31 else acc
  return out


def table_arrays(tables, codes=None):
  """ac_code (2, 256) uint16, ac_len uint8, dc_code (2, 16), dc_len of a list
  of two pairs of lengths (None: absent): canonical codewords."""
  out = {'ac_code': np.zeros((2, 256), np.uint16),
         'ac_len': np.zeros((2, 256), np.uint8),
         'dc_code': np.zeros((2, 16), np.uint16),
         'dc_len': np.zeros((2, 16), np.uint8)}
  for pair, table in enumerate(tables):
    if table is None:
      continue
    for key in ('ac', 'dc'):
      out[key + '_len'][pair] = table[key]
      for symbol, (code, _) in truth.canonical(table[key])[0].items():
        out[key + '_code'][pair, symbol] = code
  return out


# ------------------------------------------------- the sequential decoder
def _extend(value, size):
  return value if value >> (size - 1) else value - (1 << size) + 1


def _codewords(arrays, kind, t):
  """[(left-aligned 16-bit key, length, symbol)] of one table: a length above
  16 reads as 16, bits of the code above the length fall off."""
  out = []
  for s in range(arrays[kind + '_len'].shape[1]):
    length = min(int(arrays[kind + '_len'][t, s]), 16)
    if length:
      code = int(arrays[kind + '_code'][t, s]) & (1 << length) - 1
      out.append((code << (16 - length), length, s))
  return out


def shortest_codeword_rule(arrays):
  """rule(kind, t, w) -> (symbol, length) of the shortest codeword of table
  (kind, t) that the 16-bit window w starts with, (None, 0) when none does.
  In a prefix-free table it is the only one."""
  books = {(kind, t): {(length, key >> (16 - length)): s
                       for key, length, s in _codewords(arrays, kind, t)}
           for kind in ('dc', 'ac') for t in range(2)}

  def rule(kind, t, w):
    for length in range(1, 17):
      hit = books[(kind, t)].get((length, w >> (16 - length)))
      if hit is not None:
        return hit, length
    return None, 0
  return rule


def decode_table_rule(arrays, lookup_bits=9):
  """The rule of the device's decode tables, which also says what a table
  that is not prefix-free decodes to.  The codewords are sorted by (key,
  length, symbol).  Every codeword of at most lookup_bits bits claims the
  lookup entries of the prefixes that start with it, the later one in sorted
  order winning; a window whose entry is claimed takes that codeword.  Any
  other window takes the last sorted codeword whose key is <= the window, if
  the window starts with it, and nothing otherwise."""
  tables = {}
  for kind in ('dc', 'ac'):
    for t in range(2):
      entries = sorted(_codewords(arrays, kind, t))
      lookup = {}
      for key, length, s in entries:
        if length <= lookup_bits:
          first = key >> (16 - lookup_bits)
          for q in range(1 << (lookup_bits - length)):
            lookup[first + q] = (s, length)
      tables[(kind, t)] = (entries, lookup)

  def rule(kind, t, w):
    entries, lookup = tables[(kind, t)]
    hit = lookup.get(w >> (16 - lookup_bits))
    if hit is not None:
      return hit
    below = [e for e in entries if e[0] <= w]
    if not below or (below[-1][0] ^ w) >> (16 - below[-1][1]):
      return None, 0
    return below[-1][2], below[-1][1]
  return rule


def sequential_unpack(segment, slot_dc, slot_ac, arrays, rows, rule=None):
  """(levels int32 (rows, 64) with DIFF in column 0, [status0, status1,
  status2]) of the decoder include/ext/vtc_jfif_decode.h states: bits beyond
  the segment read as ones, a token must start inside the segment, the first
  malformed token stops the walk.  rule(kind, t, w): the codeword a 16-bit
  window starts with, shortest_codeword_rule(arrays) by default."""
  segment = bytes(segment)
  total = 8 * len(segment)
  padded = segment + b'\xff' * 8
  if rule is None:
    rule = shortest_codeword_rule(arrays)

  def peek(p, n):    # n <= 16 bits from bit p on
    word = int.from_bytes(padded[p >> 3:(p >> 3) + 4], 'big')
    return word >> (32 - (p & 7) - n) & (1 << n) - 1

  levels = np.zeros((rows, 64), dtype=np.int32)
  p, row = 0, 0
  while row < rows:
    slot = row % len(slot_dc)
    z = 0
    while True:
      if p >= total:
        return levels, [0, row, -1]
      if z == 0:
        s, length = rule('dc', 1 if slot_dc[slot] else 0, peek(p, 16))
        if s is None or s > 11:
          return levels, [p + 1, row, -1]
        if s:
          levels[row, 0] = _extend(peek(p + length, s), s)
        p += length + s
        z = 1
        continue
      s, length = rule('ac', 1 if slot_ac[slot] else 0, peek(p, 16))
      if s is None:
        return levels, [p + 1, row, -1]
      run, size = s >> 4, s & 15
      if size == 0:
        if s == 0x00:
          p += length
          break
        if s != 0xF0 or z + 16 > 64:
          return levels, [p + 1, row, -1]
        p += length
        z += 16
      else:
        if size > 10 or z + run > 63:
          return levels, [p + 1, row, -1]
        levels[row, z + run] = _extend(peek(p + length, size), size)
        p += length + size
        z += run + 1
      if z == 64:
        break
    row += 1
  return levels, [0, rows, p]


# ------------------------------------------------------------ constructed
def diffs_of(levels):
  """levels of one chain (row r predicted from row r - 1) with DIFF in
  column 0."""
  out = np.array(levels, dtype=np.int32)
  out[1:, 0] = out[1:, 0] - np.asarray(levels)[:-1, 0]
  return out


def chain(d):
  return np.arange(-1, d - 1, dtype=np.int32)


def one_table_layout(d):
  """What unpack_scan and dc_accumulate need of a layout, for d rows of one
  component."""
  start = np.zeros(d, dtype=np.uint8)
  start[0] = 1
  return {'rows': d, 'sampling': [(1, 1)],
          'order': np.arange(d, dtype=np.int32), 'start': start}


def pack_host(levels, tables=None):
  """(segment bytes, tables, bit offsets) of one chain of rows under table
  pair 0, by the restatement."""
  levels = np.ascontiguousarray(levels, dtype=np.int32)
  d = levels.shape[0]
  tokens = truth.scan_tokens(levels, chain(d), np.zeros(d, dtype=np.uint8))
  if tables is None:
    tables = truth.build_tables(*truth.count_symbols(tokens))
  raw, _, offsets = truth.pack_tokens(tokens, tables)
  return raw, tables, offsets


def token_spans(levels, tables):
  """[(start, end of codeword, end of value bits, ends its block)] in bits,
  of every token of one chain of rows under table pair 0."""
  levels = np.ascontiguousarray(levels, dtype=np.int32)
  d = levels.shape[0]
  codes = {key: truth.canonical(tables[0][key])[0] for key in ('dc', 'ac')}
  out, at = [], 0
  for _, block in truth.scan_tokens(levels, chain(d),
                                    np.zeros(d, dtype=np.uint8)):
    for i, (kind, symbol, _, size) in enumerate(block):
      length = codes[kind][symbol][1]
      out.append((at, at + length, at + length + size, i == len(block) - 1))
      at += length + size
  return out


def token_rows():
  """The constructed rows of tests/test_jfif_gpu.py: zero runs around the
  0xF0 boundary, every size of both signs, a coefficient at index 63 followed
  by the next block's DC, an end of block as the last bits."""
  rows = []
  for run in (15, 16, 17, 31, 32, 62):
    first = np.zeros(64, dtype=np.int32)
    first[0], first[1 + run] = 3, -2
    rows.append(first)
    if run + 3 <= 63:
      between = np.zeros(64, dtype=np.int32)
      between[1], between[2 + run] = 5, 7
      rows.append(between)
      last = np.zeros(64, dtype=np.int32)
      last[62 - run], last[63] = -1, 1
      rows.append(last)
  ac = [2 ** k - 1 for k in range(1, 11)] + [2 ** k for k in range(0, 10)]
  for sign in (1, -1):
    for at in range(0, len(ac), 9):
      row = np.zeros(64, dtype=np.int32)
      for j, m in enumerate(ac[at:at + 9]):
        row[1 + 7 * j] = sign * m
      rows.append(row)
  dc = [2 ** k - 1 for k in range(1, 12)] + [2 ** k for k in range(0, 11)]
  for m in dc:       # DIFF = m, then -m: a DC level, then 0 again
    row = np.zeros(64, dtype=np.int32)
    row[0] = m
    rows += [row, np.zeros(64, dtype=np.int32)]
  only63 = np.zeros(64, dtype=np.int32)
  only63[0], only63[63] = 4, -9
  rows.append(only63)                       # index 63, then the next DC
  dense = np.arange(64, dtype=np.int32) % 5 - 2
  dense[0] = 7
  rows.append(dense)
  rows.append(np.zeros(64, dtype=np.int32))    # an end of block, last bits
  return np.stack(rows)


def geometric_tail_tables():
  """One table pair whose AC table holds all 256 symbols with counts in a
  geometric tail: package-merge gives 16-bit codewords."""
  ac = np.array([int(1e12 * 0.9 ** i) + 1 for i in range(256)], dtype=np.int64)
  dc = np.array([int(1e6 * 0.5 ** i) + 1 for i in range(16)], dtype=np.int64)
  table = {'dc': truth.package_merge(dc), 'ac': truth.package_merge(ac)}
  assert table['ac'].max() == 16 and table['ac'].min() >= 1
  return [table, None]


# AC table of overlapping_tables(), symbol -> length.  Canonical codewords
# go by (length, symbol): 0x13 gets 111111100, the 11-bit ones follow from
# 11111110100 on, so the fifth of them, 0x22, is 11111111000.
_OVERLAP_AC = {0x00: 2, 0x01: 2, 0x02: 3, 0x03: 3, 0x11: 4, 0x07: 4, 0x08: 4,
               0x04: 5, 0x12: 6, 0x21: 7, 0x13: 9, 0x05: 11, 0x06: 11,
               0x15: 11, 0x16: 11, 0x22: 11, 0x41: 12}
OVERLAP_PREFIX, OVERLAP_LONGER = 0x14, 0x13
OVERLAP_TWIN, OVERLAP_FIRST = 0x32, 0x22


def overlapping_tables():
  """table_arrays of one pair that is not prefix-free: a canonical DC table;
  a canonical AC table plus symbol OVERLAP_PREFIX, whose codeword 11111110 is
  the head of the 9-bit codeword of OVERLAP_LONGER (both inside a 9-bit
  lookup) and of four 11-bit codewords, and plus symbol OVERLAP_TWIN under the
  11-bit codeword of OVERLAP_FIRST, which no shorter codeword is a head of."""
  ac = np.zeros(256, dtype=np.int64)
  for symbol, length in _OVERLAP_AC.items():
    ac[symbol] = length
  dc = np.array([2, 2, 2, 3, 3] + [0] * 11, dtype=np.int64)
  arrays = table_arrays([{'dc': dc, 'ac': ac}, None])
  assert arrays['ac_code'][0, OVERLAP_LONGER] == 0b111111100
  assert arrays['ac_code'][0, OVERLAP_FIRST] == 0b11111111000
  arrays['ac_len'][0, OVERLAP_PREFIX] = 8
  arrays['ac_code'][0, OVERLAP_PREFIX] = 0b11111110
  arrays['ac_len'][0, OVERLAP_TWIN] = 11
  arrays['ac_code'][0, OVERLAP_TWIN] = 0b11111111000
  return arrays


def overlapping_segment(arrays, rows, seed, tokens=11):
  """Bytes of `rows` blocks written from overlapping_tables(): a DC token,
  `tokens` AC tokens drawn from all its symbols with random value bits, an
  end of block; ones to the byte boundary.  What a decoder reads back is the
  decode rule's business: it loses its place behind the first ambiguous
  codeword and finds it again, as Huffman decoders do."""
  rs = np.random.RandomState(seed)
  # the codewords the added ones touch are written often
  symbols = sorted(set(_OVERLAP_AC) - {0x00}) + 3 * [
      OVERLAP_PREFIX, OVERLAP_LONGER, OVERLAP_TWIN, OVERLAP_FIRST, 0x05]
  bits = []

  def put(value, n):
    bits.extend(value >> (n - 1 - i) & 1 for i in range(n))

  def token(kind, symbol):
    put(int(arrays[kind + '_code'][0, symbol]),
        int(arrays[kind + '_len'][0, symbol]))
    put(int(rs.randint(0, 1 << 15)) & (1 << (symbol & 15)) - 1, symbol & 15)

  for _ in range(rows):
    token('dc', int(rs.randint(0, 5)))
    for _ in range(tokens):
      token('ac', symbols[rs.randint(0, len(symbols))])
    token('ac', 0x00)
  bits += [1] * (-len(bits) % 8)
  return np.packbits(np.array(bits, dtype=np.uint8)).tobytes()


# ------------------------------------------------------------ header bytes
def segment(marker, payload):
  return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + bytes(
      payload)


def header_parts(components=((1, 1, 1, 0),), h=8, w=8, precision=8,
                 sof=0xC0, tables=((0, 0), (1, 0)), scan_tables=None,
                 spectral=(0, 63, 0), dqt=((0, 0),), extra=b'',
                 scan_components=None):
  """The segments of a file, in order, as a list of byte strings: SOI, APP0,
  `extra`, DQT per (precision, id), SOF, DHT per (class, id), SOS; one-symbol
  Huffman tables (symbol 0, one bit), which make 0-bits a stream of empty
  blocks."""
  out = [b'\xff\xd8',
         segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00'), extra]
  for pq, tq in dqt:
    out.append(segment(0xDB, bytes([pq << 4 | tq]) + bytes([1] * (
        128 if pq else 64))))
  frame = bytes([precision]) + h.to_bytes(2, 'big') + w.to_bytes(2, 'big')
  frame += bytes([len(components)])
  for cid, ch, cv, tq in components:
    frame += bytes([cid, ch << 4 | cv, tq])
  out.append(segment(sof, frame))
  for klass, index in tables:
    out.append(segment(0xC4, bytes([klass << 4 | index]) + bytes(
        [1] + [0] * 15) + bytes([0])))
  if scan_components is None:
    scan_components = [c[0] for c in components]
  if scan_tables is None:
    scan_tables = [(0, 0)] * len(scan_components)
  scan = bytes([len(scan_components)])
  for cid, (td, ta) in zip(scan_components, scan_tables):
    scan += bytes([cid, td << 4 | ta])
  out.append(segment(0xDA, scan + bytes(spectral)))
  return out


def header_file(**kwargs):
  """A whole file around header_parts: the segment byte 0x3F holds one empty
  block (DC category 0, end of block) and six pad bits."""
  return b''.join(header_parts(**kwargs)) + b'\x3f' + b'\xff\xd9'
