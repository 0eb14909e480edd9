"""The truth of the index-decoder tests (include/vtc_index_decode.h,
utils.index_coding.unpack_index_streams), restated in a few lines of Python:
walk the bit string of every row, match the codewords of each column in turn.
Tables are {int index: str of '0' / '1'}; all comparisons are between integers
or bytes.  Shapes, tables, indices, `layout`, `image` and `gaps` are those of
tests/index_code_data.py, imported unchanged.  No GPU, no product code except
where a function says so."""
import collections

import numpy as np

import index_code_data as data

LOOKUP_BITS = 10          # VTC_INDEX_DECODE_LOOKUP_BITS, K

# all of index_code_data.SHAPES and a kmax that is no power of two
SHAPES = list(data.SHAPES) + [(7, 5, 300)]
IDS = ['%dx%d-k%d' % shape for shape in SHAPES]


def first_bad_position(tables, kmax):
  """The smallest j * kmax + i whose codeword equals another codeword of
  column j or is a prefix of one; None when every column is prefix-free.  By
  definition: a codeword that occurs twice, or that is among the proper
  prefixes of the column's codewords."""
  for j, table in enumerate(tables):
    times = collections.Counter(table.values())
    proper = {word[:n] for word in times for n in range(len(word))}
    for i in sorted(table):
      if times[table[i]] > 1 or table[i] in proper:
        return j * kmax + i
  return None


def bit_string(packed):
  packed = np.asarray(packed, dtype=np.uint8)
  return (np.unpackbits(packed) + ord('0')).astype(np.uint8).tobytes().decode()


def decode(packed, offsets, tables, kmax):
  """(indices int32 (b, m), row_bits int32 [b], malformed rows, bad position).

  Row r reads one codeword per column from bit offsets[r] on; a codeword of
  length l at position p is accepted when p + l <= min(offsets[r + 1], the
  bits of `packed`) and the bits there spell it.  A row whose offsets are
  negative or decreasing, or that finds no codeword, is malformed: the indices
  before the fault stay, the rest is -1, row_bits is what was consumed.  With
  a bad table position nothing is decoded."""
  bits = bit_string(packed)
  b, m = len(offsets) - 1, len(tables)
  indices = np.full((b, m), -1, dtype=np.int32)
  row_bits = np.zeros(b, dtype=np.int32)
  bad = first_bad_position(tables, kmax)
  if bad is not None:
    return indices, row_bits, [], bad
  # a prefix-free column has at most one codeword at a place: look the bits up
  # by length
  by_length = []
  for table in tables:
    words = {}
    for i, word in table.items():
      words.setdefault(len(word), {})[word] = i
    by_length.append(sorted(words.items()))
  malformed = []
  for r in range(b):
    start, stop = int(offsets[r]), int(offsets[r + 1])
    if start < 0 or start > stop:
      malformed.append(r)
      continue
    end, pos = min(stop, len(bits)), start
    for j in range(m):
      hit = None
      for length, words in by_length[j]:
        if pos + length <= end and bits[pos:pos + length] in words:
          hit = words[bits[pos:pos + length]]
          pos += length
          break
      if hit is None:
        malformed.append(r)
        break
      indices[r, j] = hit
    row_bits[r] = pos - start
  return indices, row_bits, malformed, None


def status(malformed, bad):
  """The int64 [3] the device reports."""
  if bad is not None:
    return [0, 0, 1 + bad]
  return [len(malformed), 1 + malformed[0] if malformed else 0, 0]


def case_stream(shape, lead):
  """(packed uint8 [nbytes], offsets int64 [b + 1]) of a shared case, built by
  data.image behind `lead` bits with data.gaps between the rows."""
  b = shape[0]
  tables, _ = data.case_tables(*shape)
  host = data.case_indices(*shape)
  offsets = data.layout(data.row_bits(host, tables), lead, data.gaps(b))
  nbytes = -(-int(offsets[-1]) // 8)
  packed, dropped = data.image(host, tables, offsets, nbytes)
  assert dropped == 0
  return packed, offsets


def long_table():
  """The 65-symbol table with every length 1 .. 64 (64 twice), built with the
  product's index_huffman_tables from data.long_weights;
  tests/test_index_code_host.py checks that construction on its own."""
  from utils import index_coding
  return index_coding.index_huffman_tables([data.long_weights()])[0]
