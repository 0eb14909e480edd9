"""The truth of the index-code tests (include/vtc_index_code.h,
utils/index_coding.py), restated in a few lines of Python: the bits of a row
are sum(len(table[j][i])), its stream is the joined strings, and the cost of a
Huffman code comes from an independent length computation (two queues over the
sorted weights).  Tables are {int index: str of '0' / '1'}; all comparisons
are between integers or bytes.  Also the shapes, tables and indices the GPU
tests share.  No GPU, no product code except where a function says so."""
import collections
import functools

import numpy as np

ABSENT = 255              # VTC_INDEX_CODE_ABSENT
MAX_COLUMNS = 4096        # VTC_INDEX_CODE_MAX_COLUMNS
MAX_SYMBOLS = 4096        # VTC_INDEX_CODE_MAX_SYMBOLS

# (b, m, kmax) at the lane, wave, chunk and block edges: one lane, one lane
# short of a wave step, a whole step, one more, past one block's first wave;
# several rows per step with idle lanes (3 -> 21 rows, 23 -> 2 rows), one row
# per step below 64 columns (42, the experiment's 41 + 1); exactly one chunk,
# one column more, three chunks with a ragged last one, the widest row.
SHAPES = [(1, 1, 4096), (63, 1, 4096), (64, 1, 4096), (65, 1, 4096),
          (257, 1, 4096), (5, 3, 16), (5, 23, 64), (257, 42, 1024),
          (3, 64, 8), (3, 65, 8), (2, 130, 8), (2, 4096, 4)]
LEADS = (0, 3, 29)


# ------------------------------------------------------------- restatement
def row_bits(indices, tables):
  """int64 [b]: sum over j of len(tables[j][indices[r, j]]); an entry the
  table lacks contributes nothing."""
  return np.array([sum(len(tables[j].get(int(i), '')) for j, i in enumerate(row))
                   for row in indices], dtype=np.int64)


def column_bits(indices, tables):
  """int64 [m]: the same lengths summed down each column."""
  return np.array([sum(len(tables[j].get(int(i), '')) for i in indices[:, j])
                   for j in range(indices.shape[1])], dtype=np.int64)


def stream(row, tables):
  return ''.join(tables[j].get(int(i), '') for j, i in enumerate(row))


def status(indices, tables):
  """[uncodable entries, 1 + the first one's flat position or 0]."""
  bad = [r * indices.shape[1] + j for r, row in enumerate(indices)
         for j, i in enumerate(row) if int(i) not in tables[j]]
  return [len(bad), 1 + bad[0] if bad else 0]


def layout(bits, lead, gaps):
  """offsets int64 [b + 1]: row r starts `lead` bits in, behind the rows
  before it and a gap of gaps[r] unused bits after each."""
  steps = np.asarray(bits, np.int64) + np.asarray(gaps, np.int64)
  return lead + np.concatenate([[0], np.cumsum(steps)]).astype(np.int64)


def image(indices, tables, offsets, nbytes):
  """The packed bytes: every row's stream at its offset, zeros elsewhere;
  what would fall past the row's window or the buffer is cut off.  Returns
  (uint8 [nbytes], bits cut off)."""
  bits = np.zeros(8 * nbytes, dtype=np.uint8)
  dropped = 0
  for r, row in enumerate(indices):
    text = stream(row, tables)
    start, stop = int(offsets[r]), int(offsets[r + 1])
    room = 0
    if 0 <= start <= stop:
      room = max(0, min(stop, 8 * nbytes) - start)
    kept = text[:room]
    dropped += len(text) - len(kept)
    bits[start:start + len(kept)] |= np.array([c == '1' for c in kept],
                                              dtype=np.uint8)
  return np.packbits(bits) if nbytes else np.zeros(0, np.uint8), dropped


def huffman_cost(weights):
  """sum(weight * codeword length) of an optimal prefix code: the sum of the
  weights of all merged nodes, by the two-queue method (the sorted leaves in
  one queue, the merged nodes, which come out in ascending order, in the
  other).  Python integers throughout."""
  leaves = collections.deque(sorted(int(w) for w in weights))
  merged = collections.deque()
  total = 0

  def lightest():
    if not merged or (leaves and leaves[0] <= merged[0]):
      return leaves.popleft()
    return merged.popleft()

  while len(leaves) + len(merged) > 1:
    node = lightest() + lightest()
    total += node
    merged.append(node)
  return total


def training_weights(counts_row, k):
  """The weights index_huffman_tables is to use: seen indices their counts,
  unseen ones below k the weight 1."""
  return [int(c) if int(c) > 0 else 1 for c in counts_row[:k]]


def table_cost(table, weights):
  return sum(int(w) * len(table[i]) for i, w in enumerate(weights))


def kraft_numerator(table):
  """sum 2^(L - len) over the codewords, L the longest: 2^L iff Kraft's sum is
  exactly 1."""
  longest = max(len(word) for word in table.values())
  return sum(1 << (longest - len(word)) for word in table.values()), longest


def entropy_bits(indices, kmax):
  """The in-sample entropy figure of the same indices, in bits."""
  total = 0.0
  for j in range(indices.shape[1]):
    counts = np.bincount(indices[:, j], minlength=kmax).astype(np.float64)
    seen = counts[counts > 0]
    total += float(-(seen * np.log2(seen / seen.sum())).sum())
  return total


# ------------------------------------------------------------------- tables
def long_weights(symbols=65):
  """2^0 .. 2^(symbols - 1): the two lightest merge first and every later
  merge takes the next leaf, so the lengths are symbols - 1 (twice),
  symbols - 2, ..., 1: with 65 symbols every length from 1 to 64."""
  return [1 << i for i in range(symbols)]


def complement(table):
  """Every bit of every codeword flipped: the same lengths, still a prefix
  code, and the long codewords are runs of ones instead of zeros."""
  flip = {ord('0'): '1', ord('1'): '0'}
  return {i: word.translate(flip) for i, word in table.items()}


def geometric_counts(seed, kmax, k):
  """A steep geometric histogram over the first k of kmax symbols, shuffled:
  about fifteen seen symbols, the rest unseen (weight 1 in training)."""
  rs = np.random.RandomState(seed)
  counts = np.zeros(kmax, dtype=np.int64)
  counts[:k] = (200000 * 0.45 ** np.arange(k)).astype(np.int64)
  counts[:k] = counts[:k][rs.permutation(k)]
  return counts


@functools.lru_cache(maxsize=None)
def case_tables(b, m, kmax):
  """(tables, k [m]) of a shape, built with the product's
  index_huffman_tables (tests/test_index_code_host.py checks that function on
  its own): column kinds in turn
    'long'   the constructed 1 .. 64-bit table, complemented so that its
             long codewords are ones (kmax >= 65 only)
    'one'    a one-symbol column, k = 1, the empty codeword
    'short'  k < kmax: the symbols from k on are absent
    'geo'    all kmax symbols, trained on geometric counts."""
  from utils import index_coding
  kinds = column_kinds(b, m, kmax)
  counts, k = [], []
  for j, kind in enumerate(kinds):
    if kind == 'long':
      row, kj = long_weights() + [0] * (kmax - 65), 65
    elif kind == 'one':
      row, kj = [7] + [0] * (kmax - 1), 1
    else:
      kj = max(2, (2 * kmax) // 3) if kind == 'short' else kmax
      row = geometric_counts(1000 * m + j, kmax, kj).tolist()
    counts.append(row)
    k.append(kj)
  tables = index_coding.index_huffman_tables(counts, k)
  return [complement(table) if kind == 'long' else table
          for kind, table in zip(kinds, tables)], k


def column_kinds(b, m, kmax):
  if m == 1:
    return ['long' if b in (63, 65) else 'geo']
  kinds = ['geo'] * m
  kinds[1] = 'one'
  kinds[2] = 'short'
  if kmax >= 65:
    kinds[0] = 'long'
  if m > 70:
    kinds[63], kinds[64] = 'one', 'short'   # either side of a chunk boundary
  return kinds


@functools.lru_cache(maxsize=None)
def case_indices(b, m, kmax):
  """int32 (b, m): every column drawn from its table's symbols, half of the
  draws by 2^-length (what the code expects), half uniform (long codewords);
  in a 'long' column the symbols of exactly 32, 33 and 64 bits are put in
  rows 0, 1 and 2 when there are that many."""
  tables, _ = case_tables(b, m, kmax)
  rs = np.random.RandomState(7 * b + 11 * m + kmax)
  out = np.zeros((b, m), dtype=np.int32)
  for j, table in enumerate(tables):
    symbols = np.array(sorted(table))
    p = np.array([2.0 ** -min(len(table[s]), 40) for s in symbols])
    likely = rs.choice(symbols, size=b, p=p / p.sum())
    uniform = rs.choice(symbols, size=b)
    out[:, j] = np.where(rs.rand(b) < 0.5, likely, uniform)
    if column_kinds(b, m, kmax)[j] == 'long':
      for r, bits in enumerate((32, 33, 64)):
        if r < b:
          out[r, j] = [s for s in symbols if len(table[s]) == bits][0]
  return out


def gaps(b):
  """Unused bits behind each row: none, a few, more than a word."""
  return [(0, 5, 1, 37, 0, 13)[r % 6] for r in range(b)]
