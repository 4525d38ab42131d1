"""CPU test of tools/dag_sched_model.py: fed the library's own tables and ticket list for the headline shape and the traced
costs, the model is a model of the traced launch -- its span, and the shape of the chain's wait for sub(j): nothing most of
the time, long stalls now and then.  The traced numbers are constants from profiles/shadow_kernel_stats.json
(``dag_trace_100000``); that launch drew its tickets at a lead of 0.2, so the model is given the order at that lead
(``OISAT_DAG_ORDER_LEAD_FAR``, which the order query alone reads), whatever the library's own lead is now.  No GPU is needed."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import dag_sched_model as model  # noqa: E402

TRACED_SPAN_MS = 51.4
TRACED_LEAD = 0.2
TRACED_COSTS = dict(far=3.65, mid=6.95, fp32=12.24, xstore=5.0, tail=20.9, diag=22.9, panel=15.3, upd=7.9, wb=3.66)


def test_model_of_the_headline_launch():
    first, far, mid, tickets = model.library_tables(720, 1440, 100000, 300.0, lead=TRACED_LEAD)
    r = model.simulate(first, far, mid, tickets, TRACED_COSTS, jitter=0.1)
    ws = r["wait_sub_us"]
    print("%d block rows, %d bulk tasks: span %.2f ms, chain step %.1f us, wait for sub(j) mean %.2f / median %.2f / max %.1f us, polling %.2f s"
          % (first.size, r["ntasks"], r["span_ms"], r["chain_step_us"], ws.mean(), np.median(ws), ws.max(), r["polling_s"]))
    assert abs(r["span_ms"] - TRACED_SPAN_MS) <= 0.1 * TRACED_SPAN_MS
    assert np.median(ws) < 1.0 and ws.mean() > 5.0
