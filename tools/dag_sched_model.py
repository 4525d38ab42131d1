"""profiling aid, CPU only: a discrete-event model of one enveloped task-graph factorization (csrc/dense_dag.inc) -- what the
launch's span is made of, and what a change of a K-block's cost or of the chain's step is worth before anybody builds it.

The envelope, the far and the middle table and the ticket list are the LIBRARY's (oisat_factor_envelope / _far / _mid,
oisat_dag_task_order_env, through tests/far_band_emul.py and tests/mid_band_emul.py); the costs are parameters, by default the
ones traced at the headline shape (profiles/shadow_kernel_stats.json, profiles/EXPERIMENTS.md "The shadow").  The model:
  * `slots` workgroup slots draw the bulk tickets in order, each the moment it is free;
  * a task's K-block k starts when both rowfin words allow it (tile (i, k) and tile (j, k) published, + one poll) and the
    blocks in front of it are done; it costs far / mid / fp32 microseconds by the row's tables, times a log-normal jitter per
    task and per block;
  * a tile task then stores X, waits for diagonal block j and needs `tail` from "T_j seen" to its publish; SUB / PRE publish
    `subtail` behind their K-loop;
  * the chain runs beside the slots on a workgroup of its own: diagonal block, wait for sub(j), panel (publishes tile
    (j+1, j)), rank-128 update, wait for pre(j+1), write-back.
usage: python tools/dag_sched_model.py [--obs 100000] [--far-us 3.65] [--mid-us 6.95] [--fp32-us 12.24] [--jitter 0.1] ..."""
import argparse
import heapq
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oi-sat-gmi_amd"), os.path.join(ROOT, "tests")]
import numpy as np

NB = 128
# microseconds, traced at the headline shape: per K-block | per task | the chain's phases
COSTS = dict(far=3.65, mid=6.95, fp32=12.24, fix=3.0, xstore=5.0, tail=20.9, subtail=4.0, poll=1.5,
             diag=22.9, panel=15.3, upd=7.9, wb=3.66)
SLOTS = 510                                                     # 2 per CU, less the chain's CU


def library_tables(ny, nx, nobs, L, swaths=True, seed=4000, lead=None):
    """(first, far, mid, tickets) of the library for a synthetic month, observations in latitude order as the plan sorts them.
    lead: the ticket lead of a far list (OISAT_DAG_ORDER_LEAD_FAR, read by the order query alone); None = the library's own."""
    from oisatgmi import dense, synthetic as syn
    import mid_band_emul as emu
    p = syn.point_obs_case(ny, nx, nobs, seed, swaths=swaths)
    lat = np.sort(np.ravel(p.obs_lat).astype(np.float64), kind="stable")
    env, far, mid = emu.tables(lat, dense.decay_constant(L))
    first = env[:far.size]
    old = os.environ.pop("OISAT_DAG_ORDER_LEAD_FAR", None)
    try:
        if lead is not None:
            os.environ["OISAT_DAG_ORDER_LEAD_FAR"] = repr(float(lead))
        return first, far, mid, emu.tickets(first, far)
    finally:
        os.environ.pop("OISAT_DAG_ORDER_LEAD_FAR", None)
        if old is not None:
            os.environ["OISAT_DAG_ORDER_LEAD_FAR"] = old


def simulate(first, far, mid, tickets, costs=COSTS, jitter=0.1, seed=0, slots=SLOTS):
    """-> dict(span_ms, chain_step_us, wait_sub_us (per step), wait_pre_us (per step), work_s, polling_s, ntasks)."""
    P = dict(COSTS)
    P.update(costs)
    nb = int(first.size)
    rng = np.random.default_rng(seed)
    inf = np.inf
    F = np.full((nb, nb), inf)                                  # F[i, k]: tile (i, k) is published; left of the envelope: at once
    for i in range(nb):
        F[i, :first[i]] = 0.0
    D = np.full(nb, inf)                                        # diagonal block j is published
    sub, pre = np.full(nb, inf), np.full(nb, inf)
    sub[0] = pre[:2] = 0.0                                      # (step 0 waits for neither)
    cstart, wait_sub, wait_pre = np.zeros(nb), np.zeros(nb), np.zeros(nb)
    chain = dict(j=0, t=0.0, phase=0)

    def chain_advance():                                        # as far as what the bulk tasks have published allows
        while chain["j"] < nb:
            j = chain["j"]
            if chain["phase"] == 0:
                cstart[j] = chain["t"]
                D[j] = chain["t"] + P["diag"]
                if j + 1 == nb:
                    chain["j"] = nb
                    return
                chain["phase"] = 1
            if chain["phase"] == 1:
                if sub[j] == inf:
                    return
                t = max(D[j], sub[j] + P["poll"] if j >= 1 else 0.0)
                wait_sub[j] = t - D[j]
                F[j + 1, j] = t + P["panel"]
                chain["t"] = t + P["panel"] + P["upd"]
                chain["phase"] = 2
            if pre[j + 1] == inf:
                return
            t = max(chain["t"], pre[j + 1] + P["poll"] if j >= 1 else 0.0)
            wait_pre[j] = t - chain["t"]
            chain.update(j=j + 1, t=t + P["wb"], phase=0)

    chain_advance()
    free = [0.0] * slots
    heapq.heapify(free)
    work = polling = 0.0
    ntasks = 0
    for word, _, i, j in tickets:
        kind = int(word) & 255
        if kind == 0:                                           # the chain's own ticket: a workgroup of its own
            continue
        ntasks += 1
        k0, kfar = (int(word) >> 8) & 1023, int(word) >> 18
        kend = j - 1 if kind == 3 else j
        kmid = min(max(int(mid[i]), kfar), max(kend, kfar))
        start = heapq.heappop(free)
        n = max(kend - k0, 0)
        busy = P["fix"]
        end = start + P["fix"]
        if n > 0:
            c = np.empty(n)
            c[:max(kfar - k0, 0)] = P["far"]
            c[max(kfar - k0, 0):max(kmid - k0, 0)] = P["mid"]
            c[max(kmid - k0, 0):] = P["fp32"]
            if jitter > 0:
                c *= rng.lognormal(0.0, jitter) * rng.lognormal(0.0, jitter, size=n)
            ready = np.maximum(F[i, k0:kend], F[j, k0:kend]) + P["poll"]
            assert ready.max() < inf, ("the ticket order is not topological", kind, i, j)
            rest = np.cumsum(c[::-1])[::-1]                     # blocks k .. kend - 1
            end = max(end + rest[0], float((ready + rest).max()))
            busy += rest[0]
        if kind == 1:
            if n > 0:
                end += P["xstore"]
                busy += P["xstore"]
            assert D[j] < inf, ("the ticket order is not topological", i, j)
            end = max(end, D[j] + P["poll"]) + P["tail"]
            busy += P["tail"]
            F[i, j] = end
        else:
            end += P["subtail"]
            busy += P["subtail"]
            (sub if kind == 2 else pre)[j] = end
        work += busy
        polling += (end - start) - busy
        heapq.heappush(free, end)
        chain_advance()
    assert chain["j"] == nb, "the chain did not finish"
    steps = slice(1, nb - 1)
    return dict(span_ms=max(max(free), D[nb - 1]) * 1e-3, chain_step_us=(cstart[nb - 1] - cstart[0]) / (nb - 1),
                wait_sub_us=wait_sub[steps], wait_pre_us=wait_pre[steps], work_s=work * 1e-6, polling_s=polling * 1e-6, ntasks=ntasks)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--grid", default="720x1440")
    ap.add_argument("--obs", type=int, default=100000)
    ap.add_argument("--L", type=float, default=300.0, help="correlation length, km")
    ap.add_argument("--slots", type=int, default=SLOTS)
    ap.add_argument("--jitter", type=float, default=0.1, help="sigma of the log-normal jitter on K-block costs (per task and per block)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lead", type=float, default=None, help="ticket lead of a far list (default: the library's kDagEnvLeadFar)")
    for k, v in COSTS.items():
        ap.add_argument("--%s-us" % k, type=float, default=v)
    a = ap.parse_args()
    ny, nx = (int(v) for v in a.grid.split("x"))
    first, far, mid, tickets = library_tables(ny, nx, a.obs, a.L, lead=a.lead)
    r = simulate(first, far, mid, tickets, {k: getattr(a, k + "_us") for k in COSTS}, a.jitter, a.seed, a.slots)
    ws, wp = r["wait_sub_us"], r["wait_pre_us"]
    print("%d block rows, %d bulk tasks on %d slots" % (first.size, r["ntasks"], a.slots))
    print("span %.2f ms; chain step %.1f us" % (r["span_ms"], r["chain_step_us"]))
    print("chain waits for sub(j): mean %.2f us, median %.2f, max %.1f; for pre(j+1): mean %.2f us" % (ws.mean(), np.median(ws), ws.max(), wp.mean()))
    print("slot work %.2f s, polling %.2f s (%.1f us per task)" % (r["work_s"], r["polling_s"], r["polling_s"] * 1e6 / r["ntasks"]))


if __name__ == "__main__":
    main()
