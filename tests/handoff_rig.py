"""What tests/test_handoff_host.py and tests/test_handoff_gpu.py share around tests/handoff_model.py: whole leader states (the
SoA dicts of oracle_lib, with the term-run table, RG_COL_RUN_COUNT and RG_COL_OUT) built from the model's per-group dicts, the
existing route -- the columns a host loads today, then RG_MF_BECOME_LEADER with m_hint = T -- and the oracle's tick over it."""
import numpy as np

import handoff_model as H
import oracle_lib as O

ALL_COLS = O.STATE_COLS + O.TERM_TABLE_COLS + ("run_count",)
SCALARS = ("commit", "term_lo", "term_hi", "dummy_index", "dummy_term", "cur_term", "run_count", "cfg")


def base_state(n_groups, P, stride):
    """Every group a quiet three-entry leader of term 2 over all P slots; RG_COL_OUT carries a pattern no tick wrote."""
    st = O.alloc_state(n_groups, P, stride)
    O.add_term_table(st)
    st["run_count"] = np.zeros(n_groups, dtype=np.uint8)
    g = np.arange(n_groups, dtype=np.uint64)
    for s in range(P):
        st["match"][s, :n_groups] = 3 if s == 0 else 2 + (g + s) % 2
        st["next"][s, :n_groups] = 4
        st["pr_commit"][s, :n_groups] = 2
        st["pflags"][:, s] = 1 | 8
    st["commit"][:], st["term_lo"][:], st["term_hi"][:], st["cur_term"][:] = 2, 1, 3, 2
    st["cfg"][:] = ((1 << P) - 1) | ((1 << P) - 1) << 24
    st["out"] = (0x01000100 + (g << 8)).astype(np.uint32)
    return st


def put_lead(st, L, d):
    P = st["n_slots"]
    for k in SCALARS:
        st[k][L] = d[k]
    for k in H.SLOT_KEYS:
        st[k][:P, L] = np.array(d[k], dtype=np.uint64)
    st["pflags"][L, :P] = d["pflags"]
    st["run_first"][:, L] = np.array(d["run_first"], dtype=np.uint64)
    st["run_term"][:, L] = np.array(d["run_term"], dtype=np.uint64)


def get_lead(st, L):
    P = st["n_slots"]
    d = {k: int(st[k][L]) for k in SCALARS}
    for k in H.SLOT_KEYS:
        d[k] = [int(x) for x in st[k][:P, L]]
    d["pflags"] = [int(x) for x in st["pflags"][L, :P]]
    d["run_first"], d["run_term"] = [int(x) for x in st["run_first"][:, L]], [int(x) for x in st["run_term"][:, L]]
    return d


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def state_with(n_groups, P, stride, cases):
    st = base_state(n_groups, P, stride)
    for c in cases:
        put_lead(st, c.L, c.lead)
    return st


def diff(a, b, cols=ALL_COLS):
    """[(column, where)] of the cells in which two states differ"""
    out = []
    for k in cols:
        x, y = a[k], b[k]
        if k in H.SLOT_KEYS or k in ("run_first", "run_term"):
            x, y = x[:, :a["n_groups"]], y[:, :a["n_groups"]]
        bad = np.argwhere(x != y)
        if len(bad):
            out.append((k, bad[:4].tolist(), [int(v) for v in x[tuple(bad[0])].ravel()[:1]], [int(v) for v in y[tuple(bad[0])].ravel()[:1]]))
    return out


def model_state(st, cases):
    """The state the model expects after promoting `cases` (the refused ones change nothing) -> (state, answers)"""
    want, answers = copy_state(st), []
    for c in cases:
        m = H.copy_lead(c.lead)
        answers.append(H.promote(c.f, m, st["n_slots"], c.persisted))
        assert answers[-1][0] == c.expect, (c.name, answers[-1])
        put_lead(want, c.L, m)
    return want, answers


def route_state(st, cases):
    """The existing route's input: the log columns and the own MATCH cell of every promoted case loaded from the arena's answer,
    and the tick that carries only RG_MF_BECOME_LEADER with m_hint = T -> (state, msgs dict)"""
    P = st["n_slots"]
    route = copy_state(st)
    msgs = O.alloc_msgs(st["n_groups"], P, st["stride"])
    for c in cases:
        if c.expect != H.DONE:
            continue
        canon = c.f.canonical()
        put_lead(route, c.L, H.existing_route(c.lead, canon, canon["last_index"] if c.persisted is None else c.persisted))
        s = H.cfg_fields(c.lead["cfg"])[2]
        msgs["m_flags"][c.L, s] = 0x02
        msgs["m_hint"][s, c.L] = c.f.term
    return route, msgs


def oracle_tick(route, msgs):
    """The reference's tick over the route state -> (state after, out words). RG_COL_RUN_COUNT is the engine's own column: derived
    here as the engine derives it."""
    cl = O.Cluster(route["n_groups"])
    cl.load_soa(route, term=2)
    gout = np.zeros(route["n_groups"], dtype=np.uint32)
    cl.tick_soa(msgs, gout)
    after = copy_state(route)
    cl.store_soa(after)
    after["run_count"] = (after["run_first"][:, :route["n_groups"]] != 0).sum(axis=0).astype(np.uint8)
    return after, gout
