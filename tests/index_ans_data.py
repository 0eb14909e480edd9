"""The truth of the range-coder tests (include/vtc_index_ans.h,
utils/index_coding.py), restated from the header in plain Python integers:
the frequencies from the counts, the 64-way interleaved rANS encoder and
decoder, the layout of a stream, and the case tables the GPU tests share.  All
comparisons are between integers or bytes.  No GPU and no product code."""
import bisect
import functools

import numpy as np

PROB_BITS = 15            # VTC_INDEX_ANS_PROB_BITS
SCALE = 1 << PROB_BITS
LANES = 64                # VTC_INDEX_ANS_LANES
LOWER = 1 << 16           # L
HEADER = 4 * LANES        # bytes of the end states
MAX_STREAM_SYMBOLS = 1 << 24
MAX_COLUMNS = 4096
MAX_SYMBOLS = 4096


# -------------------------------------------------------------- frequencies
def frequencies(counts_row, k):
  """The header's rule for one column: a list of len(counts_row) integers that
  sum to 2^15, >= 1 below k, 0 from k on."""
  kmax = len(counts_row)
  assert 1 <= k <= kmax
  w = [int(c) if int(c) > 0 else 1 for c in counts_row[:k]]
  total = sum(w)
  f = [max(1, (wi << PROB_BITS) // total) for wi in w]
  d = SCALE - sum(f)
  order = sorted(range(k), key=lambda i: (-w[i], i))
  at = 0
  while d > 0:
    f[order[at % k]] += 1
    d -= 1
    at += 1
  while d < 0:
    i = order[at % k]
    if f[i] > 1:
      f[i] -= 1
      d += 1
    at += 1
  return f + [0] * (kmax - k)


def frequency_array(counts, k=None):
  """uint16 (m, kmax) of (m, kmax) counts; k: m values, one for all, or None
  for kmax."""
  counts = np.asarray(counts)
  if counts.ndim == 1:
    counts = counts[None, :]
  m, kmax = counts.shape
  if k is None:
    k = [kmax] * m
  k = [int(v) for v in np.asarray(k).reshape(-1)]
  if len(k) == 1:
    k = k * m
  return np.array([frequencies(row.tolist(), kj)
                   for row, kj in zip(counts, k)], dtype=np.uint16)


def cumulative(freq_row):
  """Exclusive cumulative sums of one column, Python integers."""
  out, run = [], 0
  for f in freq_row:
    out.append(run)
    run += int(f)
  return out


def first_bad_column(freq):
  for j, row in enumerate(freq):
    if sum(int(f) for f in row) != SCALE:
      return j
  return None


def streams_of(b, rows):
  return -(-b // rows)


# ------------------------------------------------------------------ encoder
def encode_stream(symbols, m, freq, cum):
  """One stream: `symbols` in flat order, position t under column t % m.
  Returns (bytes, positions of the uncodable entries)."""
  count = len(symbols)
  steps = -(-count // LANES)
  kmax = len(freq[0])
  x = [LOWER] * LANES
  words = [None] * steps
  uncodable = []
  for q in reversed(range(steps)):
    emitted = []
    for lane in range(LANES):
      t = LANES * q + lane
      if t >= count:
        continue
      j, i = t % m, int(symbols[t])
      f = int(freq[j][i]) if 0 <= i < kmax else 0
      if f == 0:
        uncodable.append(t)
        continue
      c = cum[j][i]
      if x[lane] >= f << 17:
        emitted.append(x[lane] & 0xFFFF)
        x[lane] >>= 16
      x[lane] = ((x[lane] // f) << PROB_BITS) + x[lane] % f + c
      assert LOWER <= x[lane] < 1 << 32
    words[q] = emitted
  out = bytearray()
  for state in x:
    out += int(state).to_bytes(4, 'little')
  for emitted in words:
    for word in emitted:
      out += int(word).to_bytes(2, 'little')
  return bytes(out), sorted(uncodable)


def encode(indices, freq, rows):
  """(streams: list of n bytes objects, status [uncodable, 1 + first flat
  position or 0, 1 + bad column or 0]).  A bad table codes nothing: every
  stream is b''."""
  indices = np.asarray(indices)
  b, m = indices.shape
  assert rows >= 1 and rows * m <= MAX_STREAM_SYMBOLS
  n = streams_of(b, rows)
  bad = first_bad_column(freq)
  if bad is not None:
    return [b''] * n, [0, 0, 1 + bad]
  cum = [cumulative(row) for row in freq]
  table = [[int(f) for f in row] for row in freq]
  flat = indices.reshape(-1).tolist()
  streams, uncodable = [], []
  for s in range(n):
    lo, hi = s * rows * m, min(b, (s + 1) * rows) * m
    data, missing = encode_stream(flat[lo:hi], m, table, cum)
    streams.append(data)
    uncodable += [lo + t for t in missing]
  return streams, [len(uncodable), 1 + uncodable[0] if uncodable else 0, 0]


def layout(sizes, lead, gaps):
  """offsets int64 [n + 1] in bytes: stream s starts `lead` bytes in, behind
  the streams before it and gaps[s] unused bytes after each."""
  steps = np.asarray(sizes, np.int64) + np.asarray(gaps, np.int64)
  return lead + np.concatenate([[0], np.cumsum(steps)]).astype(np.int64)


def gaps(n):
  """Unused bytes behind each stream: none, odd ones, more than a word."""
  return [(0, 5, 1, 37, 0, 13)[s % 6] for s in range(n)]


def image(streams, offsets, nbytes):
  """(packed uint8 [nbytes], streams skipped): every stream at its offset,
  zeros elsewhere; a stream that does not fit its slot or the buffer is left
  out whole."""
  packed = np.zeros(nbytes, dtype=np.uint8)
  skipped = 0
  for s, data in enumerate(streams):
    start, stop = int(offsets[s]), int(offsets[s + 1])
    if start < 0 or start + len(data) > min(stop, nbytes):
      skipped += 1
      continue
    packed[start:start + len(data)] = np.frombuffer(data, dtype=np.uint8)
  return packed, skipped


# ------------------------------------------------------------------ decoder
def decode(packed, offsets, b, m, freq, rows):
  """(indices int32 (b, m), used_bytes int32 [n], status [malformed streams,
  1 + the first or 0, 1 + bad column or 0]) of the header's decoder."""
  packed = bytes(np.asarray(packed, dtype=np.uint8).tobytes())
  n = streams_of(b, rows)
  indices = np.full(b * m, -1, dtype=np.int32)
  used = np.zeros(n, dtype=np.int32)
  bad = first_bad_column(freq)
  if bad is not None:
    return indices.reshape(b, m), used, [0, 0, 1 + bad]
  cum = [cumulative(row) for row in freq]
  malformed = []
  for s in range(n):
    lo, hi = s * rows * m, min(b, (s + 1) * rows) * m
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
    for q in range(-(-count // LANES)):
      symbols, need = {}, []
      for lane in range(LANES):
        t = LANES * q + lane
        if t >= count:
          continue
        j = t % m
        at = x[lane] & (SCALE - 1)
        i = bisect.bisect_right(cum[j], at) - 1
        f = int(freq[j][i])
        assert f > 0
        x[lane] = f * (x[lane] >> PROB_BITS) + at - cum[j][i]
        assert 0 <= x[lane] < 1 << 32
        symbols[t] = i
        if x[lane] < LOWER:
          need.append(lane)
      if cursor + len(need) > room:
        dry = True      # positions from this step on stay -1
        break
      for lane in need:
        word = int.from_bytes(slot[HEADER + 2 * cursor:HEADER + 2 * cursor + 2],
                              'little')
        x[lane] = (x[lane] << 16) | word
        cursor += 1
      for t, i in symbols.items():
        indices[lo + t] = i
    used[s] = HEADER + 2 * cursor
    if dry or any(state != LOWER for state in x):
      malformed.append(s)
  return (indices.reshape(b, m), used,
          [len(malformed), 1 + malformed[0] if malformed else 0, 0])


# --------------------------------------------------------------------- rates
def ideal_bits(indices, freq):
  """sum log2(2^15 / f) of the indices under the frequencies, float64."""
  indices = np.asarray(indices)
  total = 0.0
  for j in range(indices.shape[1]):
    column = np.asarray(freq[j], dtype=np.float64)[indices[:, j]]
    total += float(np.log2(SCALE / column).sum())
  return total


def entropy_bits(indices, kmax):
  """The in-sample empirical entropy of the indices, column by column."""
  indices = np.asarray(indices)
  total = 0.0
  for j in range(indices.shape[1]):
    counts = np.bincount(indices[:, j], minlength=kmax).astype(np.float64)
    seen = counts[counts > 0]
    total += float(-(seen * np.log2(seen / seen.sum())).sum())
  return total


def total_bytes(indices, freq, rows):
  streams, status = encode(indices, freq, rows)
  assert status == [0, 0, 0]
  return sum(len(data) for data in streams)


def sparse_indices(seed, b, m, kmax=64, p_zero=0.9):
  """int32 (b, m): 0 with probability p_zero, else geometric over 1 ..
  kmax - 1 -- what the quantised codes of a sparse model look like."""
  rs = np.random.RandomState(seed)
  tail = 0.7 ** np.arange(kmax - 1)
  p = np.concatenate([[p_zero], (1 - p_zero) * tail / tail.sum()])
  return rs.choice(kmax, size=(b, m), p=p).astype(np.int32)


# the sparse scene of the rate conditions: 600 x 42 indices in ONE stream, so
# the 2048-bit flush is 0.08 bit per index against the 0.5 between the codes
RATE_SCENE = (600, 42, 64, 600)


# --------------------------------------------------------------------- cases
# (b, m, kmax, rows_per_stream): lanes that never code (1 x 1, 1 x 5); exactly
# one full step; one symbol into a second step; a lane's column changes every
# step (m = 23 and 42) with segments of 2, 2, 1 and of 100, 100, 57 rows;
# 42-symbol streams; m = 64, 65, 130, 4096; R > b.
CASES = [(1, 1, 1, 1), (1, 5, 2, 1), (64, 1, 4096, 64), (65, 1, 4096, 65),
         (5, 23, 64, 2), (257, 42, 1024, 100), (257, 42, 64, 1), (3, 64, 8, 3),
         (3, 65, 8, 2), (2, 130, 8, 2), (2, 4096, 4, 1), (5, 3, 16, 8)]
IDS = ['%dx%d-k%d-R%d' % case for case in CASES]


def column_kinds(b, m, kmax):
  """'geo'     all kmax symbols, trained on geometric counts (most symbols
               unseen: frequency 1)
     'one'     a one-symbol column, frequency 2^15: the 64-bit compare
     'short'   k < kmax: the symbols from k on are absent
     'gap'     an absent symbol between present ones (and an absent symbol 0)
     'ones'    one heavy symbol, every other at frequency 1 and in use
     'uniform' every symbol at 2^15 / kmax
     'sparse'  trained on 90 % zeros."""
  if kmax == 1:
    return ['one'] * m
  if m == 1:
    return ['uniform' if b == 64 else 'geo']
  cycle = ['geo', 'one', 'short', 'gap', 'ones', 'sparse', 'uniform']
  if kmax < 4:
    cycle = ['geo', 'one', 'ones', 'sparse']
  return [cycle[j % len(cycle)] for j in range(m)]


def _geometric_counts(seed, kmax, k):
  rs = np.random.RandomState(seed)
  counts = np.zeros(kmax, dtype=np.int64)
  counts[:k] = (200000 * 0.45 ** np.arange(k)).astype(np.int64)
  counts[:k] = counts[:k][rs.permutation(k)]
  return counts


@functools.lru_cache(maxsize=None)
def case_freq(b, m, kmax, rows):
  """uint16 (m, kmax), column kinds in turn (column_kinds)."""
  out = np.zeros((m, kmax), dtype=np.uint16)
  for j, kind in enumerate(column_kinds(b, m, kmax)):
    seed = 1000 * m + j
    if kind == 'one':
      row = [SCALE] + [0] * (kmax - 1)
    elif kind == 'uniform':
      row = [SCALE // kmax] * kmax
    elif kind == 'ones':
      row = [SCALE - (kmax - 1)] + [1] * (kmax - 1)
    elif kind == 'sparse':
      counts = np.bincount(sparse_indices(seed, 2000, 1, kmax)[:, 0],
                           minlength=kmax)
      row = frequencies(counts.tolist(), kmax)
    elif kind == 'gap':
      row = frequencies(_geometric_counts(seed, kmax, kmax).tolist(), kmax)
      row[1] += row[0] + row[2]     # symbols 0 and 2 absent, 1 and 3 present
      row[0] = row[2] = 0
    else:
      k = max(2, (2 * kmax) // 3) if kind == 'short' else kmax
      row = frequencies(_geometric_counts(seed, kmax, k).tolist(), k)
    assert sum(row) == SCALE and len(row) == kmax
    out[j] = row
  return out


@functools.lru_cache(maxsize=None)
def case_indices(b, m, kmax, rows):
  """int32 (b, m): every column drawn from its present symbols, half of the
  draws by frequency, half uniform (so frequency-1 symbols are in use)."""
  freq = case_freq(b, m, kmax, rows)
  rs = np.random.RandomState(7 * b + 11 * m + kmax + rows)
  out = np.zeros((b, m), dtype=np.int32)
  for j in range(m):
    present = np.nonzero(freq[j])[0]
    p = freq[j][present].astype(np.float64)
    likely = rs.choice(present, size=b, p=p / p.sum())
    uniform = rs.choice(present, size=b)
    out[:, j] = np.where(rs.rand(b) < 0.5, likely, uniform)
  return out


@functools.lru_cache(maxsize=None)
def case_streams(b, m, kmax, rows):
  streams, status = encode(case_indices(b, m, kmax, rows),
                           case_freq(b, m, kmax, rows), rows)
  assert status == [0, 0, 0]
  return streams
