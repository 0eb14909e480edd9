"""Writes tests/golden/quantization.npz: the expected outputs of the
quantisation tests for the seeded inputs of tests/quantization_data.py.

  python tools/make_quantization_golden.py

The truth is the float64 numpy restatement of include/vtc_quant.h in
tests/quantization_data.py (the reference never shipped utils.quantization).
Runs on the CPU.  Before writing, it asserts the conditions that keep the
fixture discriminating (quantization_data.check_conditions):
  - in every fit, for every element and every iteration, the second-best cost
    exceeds the best by more than 1e-8 * (1 + best), so that a codebook or a
    length that is off by the tests' 1e-11 cannot flip an assignment;
  - every convergence test (J_prev - J) is more than 1e-6 * epsilon * J_prev
    away from epsilon * J_prev;
  - a column loses a codeword; a column converges early and one does not;
  - a fit with lambda > 0 moves an assignment away from the nearest codeword.
"""
import pathlib
import sys

import numpy as np

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'tests'))
sys.path.insert(0, str(REPO / 'vision-transform-codes_amd'))
import quantization_data as data  # noqa: E402


def narrow(a):
  for dtype in (np.int8, np.int16, np.int32):
    if a.min(initial=0) >= np.iinfo(dtype).min and (
        a.max(initial=0) <= np.iinfo(dtype).max):
      return a.astype(dtype)
  return a


def main():
  out = {}
  results = {name: data.run_fit(name) for name in sorted(data.FITS)}
  facts = data.conditions(results)
  data.check_conditions(facts)
  for name, (state, history, _) in results.items():
    for key, value in state.items():
      out['%s_%s' % (name, key)] = (narrow(value) if key in data.STATE_INT
                                    else value)
  for key, value in facts.items():
    out['fact_' + key] = np.float64(value)

  # uniform codebooks and their zero points, written out independently of
  # utils.quantization: a Python loop per column
  books = []
  for lo, hi, w in zip(data.UNIFORM_LO, data.UNIFORM_HI, data.UNIFORM_W):
    lo, hi = (0.0, 0.0) if np.isnan(lo) else (lo, hi)
    m_lo, m_hi = int(np.rint(lo / w)), int(np.rint(hi / w))
    books.append([m * w for m in range(m_lo, m_hi + 1)])
  kmax = max(len(book) for book in books)
  out['uniform_codebooks'] = np.array(
      [book + [np.inf] * (kmax - len(book)) for book in books])
  out['uniform_k'] = narrow(np.array([len(book) for book in books]))
  out['uniform_zero'] = narrow(np.array(
      [book.index(0.0) if 0.0 in book else -1 for book in books]))

  path = REPO / 'tests' / 'golden' / 'quantization.npz'
  np.savez_compressed(path, **out)
  print('wrote %s: %d arrays, %d bytes' % (path, len(out),
                                           path.stat().st_size))
  print('facts', facts)


if __name__ == '__main__':
  main()
