"""
Zig-zag scan of a matrix and its inverse, on the host in numpy: the reference's
utils/matrix_zigzag.py (`zigzag`, `inverse_zigzag`), same names, arguments and
float64 results.

Both walk one list of positions, scan_positions(vmax, hmax): from (0, 0),
anti-diagonals with an even row + column sum are walked upwards to the right,
the odd ones downwards to the left; a walk that reaches the top row steps
right, one that reaches the last column steps down, one that reaches the
bottom row steps right and one that reaches the first column steps down.  For
8 x 8 this is the scan of ITU-T T.81 figure A.6.

The reference looks at the top row before the last column when it walks
upwards, so on a shape whose top right corner lies on an even diagonal (an odd
number of columns above more than one row, e.g. 3 x 5) its walk steps out of
the matrix there and ends: the positions it has not visited keep the zeros
both functions start from.  scan_positions ends in the same place, because the
callers' data was laid out by that scan.
"""
import numpy as np


def scan_positions(vmax, hmax):
  """[(row, column), ...] in scan order; shorter than vmax * hmax where the
  reference's walk ends early (see the module text)."""
  positions = []
  v = h = 0
  while v < vmax and h < hmax:
    positions.append((v, h))
    if (v + h) % 2 == 0:        # upwards
      if v == 0:
        h += 1
      elif h == hmax - 1:
        v += 1
      else:
        v, h = v - 1, h + 1
    else:                       # downwards
      if v == vmax - 1:
        h += 1
      elif h == 0:
        v += 1
      else:
        v, h = v + 1, h - 1
    if (v, h) == (vmax - 1, hmax - 1):
      positions.append((v, h))
      break
  return positions


def zigzag(input):
  """1-d float64 array of input.shape[0] * input.shape[1] entries: the entries
  of the 2-d `input` in scan order."""
  input = np.asarray(input)
  vmax, hmax = input.shape[0], input.shape[1]
  output = np.zeros(vmax * hmax)
  for i, (v, h) in enumerate(scan_positions(vmax, hmax)):
    output[i] = input[v, h]
  return output


def inverse_zigzag(input, vmax, hmax):
  """(vmax, hmax) float64 matrix whose scan is the 1-d `input`."""
  output = np.zeros((vmax, hmax))
  for i, (v, h) in enumerate(scan_positions(vmax, hmax)):
    output[v, h] = input[i]
  return output


def scan_order(vmax, hmax):
  """int32 `order` for utils.jpeg.quantize: scan position k reads the flattened
  (row-major) coefficient order[k].  Full shapes only."""
  positions = scan_positions(vmax, hmax)
  assert len(positions) == vmax * hmax, 'the scan of this shape ends early'
  return np.array([v * hmax + h for v, h in positions], dtype=np.int32)
