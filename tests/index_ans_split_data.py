"""The truth of the split range-coder tests (include/ext/vtc_index_ans_split.h,
utils/index_coding.py), restated from the header in plain Python integers: the
two tables from the counts, the 64-way interleaved encoder and decoder that
code every index as hi = i >> 8 and lo = i & 255, the status words, and the
case tables the GPU tests share.  The primitives, the layout helpers and the
frequency rule of one table are those of tests/index_ans_data.py.  All
comparisons are between integers or bytes.  No GPU and no product code."""
import bisect
import functools

import numpy as np

import index_ans_data as base

PROB_BITS, SCALE, LANES = base.PROB_BITS, base.SCALE, base.LANES
LOWER, HEADER = base.LOWER, base.HEADER
MAX_STREAM_SYMBOLS = base.MAX_STREAM_SYMBOLS
MAX_SYMBOLS = 131072      # VTC_INDEX_ANS_SPLIT_MAX_SYMBOLS
LO_BITS = 8               # VTC_INDEX_ANS_SPLIT_LO_BITS
LO = 1 << LO_BITS

layout, gaps, image, streams_of = (base.layout, base.gaps, base.image,
                                   base.streams_of)


def hi_symbols(kmax):
  return -(-kmax // LO)


# -------------------------------------------------------------- frequencies
def frequencies(counts, k=None):
  """(freq_hi uint16 [H], freq_lo uint16 (H, 256)) of the [kmax] counts with k
  codewords in use: the header's rule."""
  counts = [int(c) for c in counts]
  kmax = len(counts)
  k = kmax if k is None else int(k)
  assert 1 <= k <= kmax <= MAX_SYMBOLS
  top = hi_symbols(kmax)
  freq_hi = np.zeros(top, dtype=np.uint16)
  freq_lo = np.zeros((top, LO), dtype=np.uint16)
  weights = []
  for h in range(hi_symbols(k)):
    block = counts[LO * h:LO * (h + 1)]
    block += [0] * (LO - len(block))
    k_h = min(LO, k - LO * h)
    freq_lo[h] = base.frequencies(block, k_h)
    weights.append(sum(c if c > 0 else 1 for c in block[:k_h]))
  # steps 2 and 3 on the block weights: they are positive, so step 1 of the
  # one-table rule leaves them alone
  freq_hi[:len(weights)] = base.frequencies(weights, len(weights))
  return freq_hi, freq_lo


def bad_table(freq_hi, freq_lo, kmax):
  """status[2]: 0, 1 for a bad freq_hi, else 2 + the smallest bad row."""
  if sum(int(f) for f in freq_hi) != SCALE:
    return 1
  for h in range(hi_symbols(kmax)):
    if int(freq_hi[h]) == 0:
      continue
    row = [int(f) for f in freq_lo[h]]
    if sum(row) != SCALE or any(f for l, f in enumerate(row)
                                if LO * h + l >= kmax):
      return 2 + h
  return 0


class Tables(object):
  """Python integers of a checked pair of tables and their cumulative sums."""

  def __init__(self, freq_hi, freq_lo, kmax):
    self.kmax = kmax
    self.f_hi = [int(f) for f in freq_hi]
    self.c_hi = base.cumulative(self.f_hi)
    self.f_lo, self.c_lo = {}, {}
    for h, f in enumerate(self.f_hi):
      if f:
        self.f_lo[h] = [int(v) for v in freq_lo[h]]
        self.c_lo[h] = base.cumulative(self.f_lo[h])

  def symbols(self, i):
    """((f, c) of lo, (f, c) of hi) or None for an uncodable entry."""
    if not 0 <= i < self.kmax:
      return None
    hi, lo = i >> LO_BITS, i & (LO - 1)
    if self.f_hi[hi] == 0 or self.f_lo[hi][lo] == 0:
      return None
    return ((self.f_lo[hi][lo], self.c_lo[hi][lo]),
            (self.f_hi[hi], self.c_hi[hi]))


# ------------------------------------------------------------------ encoder
def _put(x, lane, f, c, emitted):
  if x[lane] >= f << 17:
    emitted.append(x[lane] & 0xFFFF)
    x[lane] >>= 16
  x[lane] = ((x[lane] // f) << PROB_BITS) + x[lane] % f + c
  assert LOWER <= x[lane] < 1 << 32


def encode_stream(symbols, tables):
  """One stream.  Returns (bytes, positions of the uncodable entries)."""
  count = len(symbols)
  steps = -(-count // LANES)
  x = [LOWER] * LANES
  words = [None] * steps
  uncodable = []
  for q in reversed(range(steps)):
    entries = {}
    for lane in range(LANES):
      t = LANES * q + lane
      if t >= count:
        continue
      pair = tables.symbols(int(symbols[t]))
      if pair is None:
        uncodable.append(t)
      else:
        entries[lane] = pair
    phase_b, phase_a = [], []
    for lane in sorted(entries):          # lo for all lanes ...
      _put(x, lane, entries[lane][0][0], entries[lane][0][1], phase_b)
    for lane in sorted(entries):          # ... then hi for all lanes
      _put(x, lane, entries[lane][1][0], entries[lane][1][1], phase_a)
    words[q] = phase_a + phase_b          # as the decoder reads them
  out = bytearray()
  for state in x:
    out += int(state).to_bytes(4, 'little')
  for emitted in words:
    for word in emitted:
      out += int(word).to_bytes(2, 'little')
  return bytes(out), sorted(uncodable)


def encode(indices, freq_hi, freq_lo, kmax, rows):
  """(streams: list of n bytes objects, status [uncodable, 1 + first row or 0,
  the bad-table word]).  A bad table codes nothing: every stream is b''."""
  flat = np.asarray(indices).reshape(-1).tolist()
  b = len(flat)
  assert 1 <= rows <= MAX_STREAM_SYMBOLS and 1 <= kmax <= MAX_SYMBOLS
  n = streams_of(b, rows)
  bad = bad_table(freq_hi, freq_lo, kmax)
  if bad:
    return [b''] * n, [0, 0, bad]
  tables = Tables(freq_hi, freq_lo, kmax)
  streams, uncodable = [], []
  for s in range(n):
    lo, hi = s * rows, min(b, (s + 1) * rows)
    data, missing = encode_stream(flat[lo:hi], tables)
    streams.append(data)
    uncodable += [lo + t for t in missing]
  return streams, [len(uncodable), 1 + uncodable[0] if uncodable else 0, 0]


# ------------------------------------------------------------------ decoder
def _get(x, lane, f_row, c_row):
  at = x[lane] & (SCALE - 1)
  i = bisect.bisect_right(c_row, at) - 1
  f = f_row[i]
  assert f > 0
  x[lane] = f * (x[lane] >> PROB_BITS) + at - c_row[i]
  assert 0 <= x[lane] < 1 << 32
  return i


def decode(packed, offsets, b, freq_hi, freq_lo, kmax, rows):
  """(indices int32 [b], used_bytes int32 [n], status [malformed streams,
  1 + the first or 0, the bad-table word]) of the header's decoder."""
  packed = bytes(np.asarray(packed, dtype=np.uint8).tobytes())
  n = streams_of(b, rows)
  indices = np.full(b, -1, dtype=np.int32)
  used = np.zeros(n, dtype=np.int32)
  bad = bad_table(freq_hi, freq_lo, kmax)
  if bad:
    return indices, used, [0, 0, bad]
  tables = Tables(freq_hi, freq_lo, kmax)
  malformed = []
  for s in range(n):
    lo, hi = s * rows, min(b, (s + 1) * rows)
    count = hi - lo
    start, after = int(offsets[s]), int(offsets[s + 1])
    stop = min(after, len(packed))
    if start < 0 or start > after or stop - start < HEADER:
      malformed.append(s)
      continue
    slot = packed[start:stop]
    x = [int.from_bytes(slot[4 * l:4 * l + 4], 'little') for l in range(LANES)]
    room = (len(slot) - HEADER) // 2
    cursor, dry = 0, False

    def refill(need, cursor):
      if cursor + len(need) > room:
        return None
      for lane in need:
        at = HEADER + 2 * cursor
        x[lane] = (x[lane] << 16) | int.from_bytes(slot[at:at + 2], 'little')
        cursor += 1
      return cursor

    for q in range(-(-count // LANES)):
      lanes = [l for l in range(LANES) if LANES * q + l < count]
      his = {l: _get(x, l, tables.f_hi, tables.c_hi) for l in lanes}   # A
      after_a = refill([l for l in lanes if x[l] < LOWER], cursor)
      if after_a is None:
        dry = True      # positions from this step on stay -1
        break
      los = {l: _get(x, l, tables.f_lo[his[l]], tables.c_lo[his[l]])
             for l in lanes}                                           # B
      after_b = refill([l for l in lanes if x[l] < LOWER], after_a)
      if after_b is None:
        dry = True      # the words of its phase A do not count either
        break
      cursor = after_b
      for l in lanes:
        indices[lo + LANES * q + l] = LO * his[l] + los[l]
        assert 0 <= indices[lo + LANES * q + l] < kmax
    used[s] = HEADER + 2 * cursor
    if dry or any(state != LOWER for state in x):
      malformed.append(s)
  return indices, used, [len(malformed),
                         1 + malformed[0] if malformed else 0, 0]


# --------------------------------------------------------------------- rates
def ideal_bits(indices, freq_hi, freq_lo):
  """sum log2(2^15 / f_hi) + log2(2^15 / f_lo) of the indices, float64."""
  flat = np.asarray(indices).reshape(-1).astype(np.int64)
  f_hi = np.asarray(freq_hi, dtype=np.float64)[flat >> LO_BITS]
  f_lo = np.asarray(freq_lo, dtype=np.float64).reshape(-1)[flat]
  return float(np.log2(SCALE / f_hi).sum() + np.log2(SCALE / f_lo).sum())


def entropy_bits(indices, kmax):
  return base.entropy_bits(np.asarray(indices).reshape(-1, 1), kmax)


def sparse_indices(seed, b, k, p_zero):
  """int32 [b]: 0 with probability p_zero, else a Zipf tail over 1 .. k - 1 in
  a scrambled order -- what the index of a vector quantiser of sparse codes
  looks like."""
  rs = np.random.RandomState(seed)
  tail = 1.0 / np.arange(1, k)
  names = 1 + rs.permutation(k - 1)
  p = (1 - p_zero) * tail / tail.sum()
  out = np.zeros(b, dtype=np.int32)
  draw = rs.rand(b) >= p_zero
  out[draw] = names[rs.choice(k - 1, size=int(draw.sum()), p=p / p.sum())]
  return out


# (b, k, kmax, p_zero): the scenes of the cost bound, trained in sample
SCENES = [(50000, 20000, 32768, 0.9), (100000, 100000, 131072, 0.5),
          (3000, 5000, 5000, 0.9)]


# --------------------------------------------------------------------- cases
# (b, kmax, rows_per_stream): b 1, 63, 64, 65, 129, 300; R 1, 64, 100, > b;
# kmax 1, 2, 255, 256, 257, 4096, 4097, 65 536, 131 072
CASES = [(1, 1, 1), (63, 2, 64), (64, 255, 64), (65, 256, 100),
         (129, 257, 64), (300, 4096, 100), (300, 4097, 1000), (65, 65536, 1),
         (300, 131072, 100), (129, 131072, 64), (300, 5000, 100)]
IDS = ['%d-k%d-R%d' % case for case in CASES]


@functools.lru_cache(maxsize=None)
def case_tables(b, kmax, rows):
  """Tables trained on a sparse scene of the case's kmax, k = kmax: most
  symbols unseen, so frequency-1 symbols abound."""
  if kmax == 1:
    return frequencies([0], 1)
  train = sparse_indices(31 * kmax + b, 2000, kmax, 0.5)
  return frequencies(np.bincount(train, minlength=kmax).tolist(), kmax)


@functools.lru_cache(maxsize=None)
def case_indices(b, kmax, rows):
  """int32 [b]: a third drawn as the training scene, a third uniform over all
  kmax symbols (frequency-1 symbols, the last, partial block), a third from
  the last block."""
  rs = np.random.RandomState(7 * b + kmax + rows)
  if kmax == 1:
    return np.zeros(b, dtype=np.int32)
  likely = sparse_indices(17 * kmax + b, b, kmax, 0.5)
  uniform = rs.randint(0, kmax, size=b)
  last = rs.randint(LO * (hi_symbols(kmax) - 1), kmax, size=b)
  pick = rs.randint(0, 3, size=b)
  out = np.where(pick == 0, likely, np.where(pick == 1, uniform, last))
  out = out.astype(np.int32)
  out[0] = kmax - 1          # never the poison pattern, always the last symbol
  return out


@functools.lru_cache(maxsize=None)
def case_streams(b, kmax, rows):
  freq_hi, freq_lo = case_tables(b, kmax, rows)
  streams, status = encode(case_indices(b, kmax, rows), freq_hi, freq_lo,
                           kmax, rows)
  assert status == [0, 0, 0]
  return streams


def hand_tables():
  """name -> (freq_hi, freq_lo, kmax, indices): hand-made tables, each with
  indices that its present symbols can code.
    'short'    k < kmax: the symbols from k on are absent
    'hi-gap'   a zero freq_hi between used rows, whose lo row is garbage
    'lo-gap'   an absent lo symbol between present ones, and an absent lo 0
    'ones'     frequency-1 symbols in use, in both tables
    'single'   a one-symbol hi with a one-symbol lo: costs no words
    'partial'  indices that land in the last, partial block"""
  rs = np.random.RandomState(5)
  out = {}
  counts = rs.randint(0, 9, size=1000)
  freq_hi, freq_lo = frequencies(counts.tolist(), 700)
  out['short'] = (freq_hi, freq_lo, 1000, rs.randint(0, 700, size=200))

  freq_hi = np.array([SCALE - 300, 0, 300], np.uint16)
  freq_lo = np.zeros((3, LO), np.uint16)
  freq_lo[0] = base.frequencies(rs.randint(1, 50, size=LO).tolist(), LO)
  freq_lo[1] = 65535                         # never read
  freq_lo[2] = base.frequencies(rs.randint(1, 50, size=LO).tolist(), LO)
  picks = np.concatenate([rs.randint(0, LO, size=100),
                          rs.randint(2 * LO, 3 * LO, size=100)])
  out['hi-gap'] = (freq_hi, freq_lo, 3 * LO, rs.permutation(picks))

  freq_hi = np.array([SCALE // 2, SCALE // 2], np.uint16)
  freq_lo = np.zeros((2, LO), np.uint16)
  freq_lo[0, [1, 3, 200]] = [100, SCALE - 300, 200]
  freq_lo[1, [0, 2, 255]] = [SCALE - 2, 1, 1]
  out['lo-gap'] = (freq_hi, freq_lo, 2 * LO,
                   rs.choice([1, 3, 200, 256, 258, 511], size=200))

  top = 40
  freq_hi = np.array([SCALE - (top - 1)] + [1] * (top - 1), np.uint16)
  freq_lo = np.zeros((top, LO), np.uint16)
  freq_lo[:, 0] = SCALE - (LO - 1)
  freq_lo[:, 1:] = 1
  out['ones'] = (freq_hi, freq_lo, top * LO,
                 rs.randint(0, top * LO, size=200))

  freq_hi = np.array([0, SCALE, 0], np.uint16)
  freq_lo = np.zeros((3, LO), np.uint16)
  freq_lo[1, 7] = SCALE
  out['single'] = (freq_hi, freq_lo, 3 * LO, np.full(200, LO + 7))

  kmax = 4 * LO + 5
  freq_hi, freq_lo = frequencies(rs.randint(0, 3, size=kmax).tolist(), kmax)
  out['partial'] = (freq_hi, freq_lo, kmax,
                    rs.randint(4 * LO, kmax, size=200))
  return {name: (fh, fl, kmax, np.asarray(host, np.int32))
          for name, (fh, fl, kmax, host) in out.items()}
