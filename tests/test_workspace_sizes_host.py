"""Every vtc_*_workspace_bytes query answers what tests/golden/
workspace_sizes.txt recorded (tools/make_golden_workspace_sizes.py, on the
commit before the layouts moved into one type per route).  The grid stands on
both sides of every route switch and includes empty and invalid shapes.

No GPU needed: the queries are host-only, and with no device the compute-unit
count falls back to 256, the MI355X count."""
import importlib.util
import pathlib
import re

REPO = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = REPO / 'tests' / 'golden' / 'workspace_sizes.txt'
HEADER = REPO / 'include' / 'vtc_hip.h'


def _recorder():
  spec = importlib.util.spec_from_file_location(
      'make_golden_workspace_sizes',
      REPO / 'tools' / 'make_golden_workspace_sizes.py')
  module = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(module)
  return module


def _lines():
  out = []
  for raw in GOLDEN.read_text().splitlines():
    call, value = raw.split(' = ')
    name, *args = call.split()
    out.append((name, tuple(args), int(value), raw))
  return out


def declared_queries():
  text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
  return sorted(set(re.findall(r'\b(vtc_[a-z0-9_]+_workspace_bytes)\s*\(',
                               text)))


def test_every_declared_query_has_recorded_lines():
  recorded = {name for name, _, _, _ in _lines()}
  queries = declared_queries()
  assert len(queries) >= 17
  for name in queries:
    assert name in recorded, name + ' has no line in ' + GOLDEN.name
  assert recorded <= set(queries)


def test_recorded_grid_is_the_recorders_grid():
  """The file was not thinned: it holds exactly the calls the recorder makes."""
  grid = [(name, tuple(repr(a) if isinstance(a, float) else str(a)
                       for a in args))
          for name, args in _recorder().grid()]
  assert [(name, args) for name, args, _, _ in _lines()] == grid


def test_every_query_answers_the_recorded_size():
  import vtc_hip
  lib = vtc_hip.load_library()
  call = _recorder().call
  wrong = []
  for name, args, want, raw in _lines():
    got = call(lib, name, args)
    if got != want:
      wrong.append('%s  (now %d)' % (raw, got))
  assert not wrong, '%d of the recorded sizes changed:\n%s' % (
      len(wrong), '\n'.join(wrong[:40]))
