"""Writes tests/golden/nettrace_lossy.txt: montecarlo.format_trace of
montecarlo.trace_net_host for the instance test_montecarlo_nettrace.format_case
picks (a lost send, a lost commander packet and its 'no packet arrived').  Run
from tests/; the text was read line by line against the event definition
before it was committed, so a regenerated file that differs is a change of the
format or of the specification, not a refresh."""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

from conftest import sub  # noqa: E402
from test_montecarlo_nettrace import format_case  # noqa: E402

n, row, counts, events = format_case()
(HERE / "nettrace_lossy.txt").write_text(sub("montecarlo").format_trace(n, row, counts, events) + "\n")
