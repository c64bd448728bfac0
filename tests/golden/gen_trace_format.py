"""Writes tests/golden/trace_honest.txt and trace_failed.txt: montecarlo.format_trace
of montecarlo.trace_host for the two instances test_montecarlo_trace.FORMAT_CASES
names (sizeL 8 under seed 2768, the C twin's samples).  Run from tests/; the
texts were read line by line against the event definition before they were
committed, so a regenerated file that differs is a change of the format or of
the specification, not a refresh."""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

from conftest import sub  # noqa: E402
from test_montecarlo_adversary import HostEngine  # noqa: E402
from test_montecarlo_trace import FORMAT_CASES, SIZEL  # noqa: E402

mc = sub("montecarlo")
for name, (n, nd, idx, word) in FORMAT_CASES.items():
    rows, counts, events = mc.trace_host(n, SIZEL, nd, idx, 2768, HostEngine(), adversary=word)
    (HERE / f"trace_{name}.txt").write_text(mc.format_trace(n, rows[0], counts[0], events[0]) + "\n")
