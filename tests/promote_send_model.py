"""The promotion into an engine with device Inflights (include/raftgroups_handoff.h) as a literal Python model of ONE group:
handoff_model.promote -- Raft::become_leader (src/raft.rs:1151-1202) with Raft::reset (:942-971) --, then what the reference does
to the Inflights in reset and the bcast_append that follows become_leader (:2190-2191). Citations: pingcap/raft-rs v0.6.0.

The leader side is handoff_model's dict of one group's columns plus

    windows      a list of P Inflights, each the list of its entries oldest first (None for a slot without a Progress)
    sizes        {index: Entry::compute_size()} of the log's entries, for Config::max_size_per_msg (only what is looked up is needed)

The send decision is written as the reference writes it -- is_paused, the entries slice with both limits, update_state, the loop of
bcast_append over the Progress map -- NOT as the closed form csrc/rg_promote.h derives from it: the two are independent
restatements, and tests/test_promote_send_host.py holds them (and the oracle's own stage) against each other."""
import handoff_model as H

PF_PAUSED, PF_INS_FULL = 0x04, 0x10
SEND_APPEND = 1
NO_LIMIT = (1 << 64) - 1
WINDOW_SHAPES = ("empty", "compact", "ring", "wrapped", "full")


def varint_len(v):
    """prost::encoding::encoded_len_varint"""
    n = 1
    while v >= 0x80:
        v >>= 7
        n += 1
    return n


def empty_entry_size(term, index):
    """Entry::compute_size() of Entry { entry_type: EntryNormal, term, index, data: [], context: [] } (eraftpb.proto: term = 2,
    index = 3): a field holding its default is not encoded, each of the others costs its tag byte and its varint."""
    return (1 + varint_len(term) if term else 0) + (1 + varint_len(index) if index else 0)


def limit_size(sizes, max_bytes):
    """util::limit_size (src/util.rs:52-76) over a list of entry sizes -> how many are kept"""
    if len(sizes) <= 1 or max_bytes == NO_LIMIT:
        return len(sizes)
    size, n = 0, 0
    for s in sizes:
        if size == 0:  # the first entry always (and any entry behind a prefix of empty ones)
            size += s
            n += 1
            continue
        size += s
        if size > max_bytes:
            break
        n += 1
    return n


def is_paused(pb, window, cap):
    """Progress::is_paused (src/tracker/progress.rs:210-216)"""
    state = pb & H.PF_STATE_MASK
    if state == H.PROBE:
        return bool(pb & PF_PAUSED)
    if state == H.REPLICATE:
        return len(window) == cap  # ins.full()
    return True  # Snapshot


def maybe_send_append(lead, windows, s, allow_empty, cap, max_entries, max_bytes, sizes):
    """Raft::maybe_send_append(to, pr, allow_empty) (src/raft.rs:773-819) for slot s -> a message (prev_index, n_entries) or None.
    The term lookup cannot fail here (next - 1 >= first_index - 1) and pending_request_snapshot is 0 behind a reset."""
    pb = lead["pflags"][s]
    if is_paused(pb, windows[s], cap):  # :779-787
        return None
    nxt, last = lead["next"][s], lead["term_hi"]
    assert lead["pend_rs"][s] == 0 or not pb & H.PF_PEND_RS
    assert nxt >= lead["dummy_index"] + 1, "RaftLog::entries: Compacted"
    ents = list(range(nxt, last + 1))  # RaftLog::entries(next, max_size) (raft_log.rs:382-389) ...
    if max_bytes is not None:
        ents = ents[:limit_size([sizes[i] for i in ents], max_bytes)]  # ... limited in bytes (util::limit_size)
    elif max_entries and len(ents) > max_entries:
        ents = ents[:max_entries]  # ... or in entries (the engine's other form of the limit)
    if not allow_empty and not ents:  # :800-802
        return None
    # prepare_send_entries (:722-731): m.index = pr.next_idx - 1, then pr.update_state(last) (progress.rs:231-243)
    if ents:
        state = pb & H.PF_STATE_MASK
        if state == H.REPLICATE:
            lead["next"][s] = ents[-1] + 1  # optimistic_update
            windows[s].append(ents[-1])     # ins.add(last)
        elif state == H.PROBE:
            lead["pflags"][s] = pb | PF_PAUSED  # pause()
        else:
            raise AssertionError("sending append in unhandled state")
    return (nxt - 1, len(ents))


def promote_send(node, lead, windows, P, cap, persisted=None, max_entries=0, max_bytes=None, esz=None, esz_w=0):
    """One record of rgh_follow_promote* -> (answer of handoff_model.promote, items [(slot, kind, prev_index, last_index, n_msgs)]).
    `lead` and `windows` change only where the status is DONE; `esz` (the group's row of cumulative sizes, a list of esz_w u32
    cells, or None) gets the record of the empty entry."""
    a = H.promote(node, lead, P, persisted)
    if a[0] != H.DONE:
        return a, []
    _, _, self_slot, _, present = H.cfg_fields(lead["cfg"])
    term, hi = a[1], a[2]
    # Raft::reset (raft.rs:959-966): every Progress of the tracker = Progress::new(last_index + 1, max_inflight) -- a new, empty
    # Inflights (Progress::reset -> ins.reset(), progress.rs:82-92; inflights.rs:121-124), the leader's own included
    for s in range(P):
        if present >> s & 1:
            windows[s] = []
    sizes = {hi: empty_entry_size(term, hi)}
    if esz is not None:  # the cumulative size record of the entry become_leader appended (:1191-1194)
        esz[hi & (esz_w - 1)] = (esz[(hi - 1) & (esz_w - 1)] + sizes[hi]) & 0xFFFFFFFF
    # bcast_append (raft.rs:857-864): send_append(to) = maybe_send_append(to, pr, true) for every Progress but the own, then --
    # as the stage does behind any send -- `while maybe_send_append(to, false)` (the ack loop's form, :1745-1761): it finds the
    # peer paused
    items = []
    for s in range(P):
        if not present >> s & 1 or s == self_slot:
            continue
        msgs = []
        m = maybe_send_append(lead, windows, s, True, cap, max_entries, max_bytes, sizes)
        while m is not None:
            msgs.append(m)
            m = maybe_send_append(lead, windows, s, False, cap, max_entries, max_bytes, sizes)
        if msgs:
            assert all(msgs[k + 1][0] == msgs[k][0] + msgs[k][1] for k in range(len(msgs) - 1))
            items.append((s, SEND_APPEND, msgs[0][0], msgs[-1][0] + msgs[-1][1], len(msgs)))
    for s in range(P):  # RG_PF_INS_FULL is the engine's copy of ins.full() of a Replicate peer
        if present >> s & 1:
            pb = lead["pflags"][s] & ~PF_INS_FULL
            full = (pb & H.PF_STATE_MASK) == H.REPLICATE and len(windows[s]) == cap
            lead["pflags"][s] = pb | (PF_INS_FULL if full else 0)
    return a, items


def window_of(shape, cap, base=10):
    """A window of one of the five starting shapes as (start, [entries oldest first]) for rg_load_inflights: empty; compact (up to
    four entries, fewer where cap is smaller); ring (more than four, where cap allows: else the largest count below cap); wrapped
    (start near the end of the ring); full (count == cap)."""
    if shape == "empty":
        return 0, []
    if shape == "compact":
        n = max(1, min(3, cap - 1)) if cap > 1 else 1
        return 0, [base + 2 * i for i in range(n)]
    if shape == "ring":
        n = max(1, min(6, cap - 1)) if cap > 1 else 1
        return 0, [base + 3 * i for i in range(n)]
    if shape == "wrapped":
        n = max(1, min(6, cap - 1)) if cap > 1 else 1
        return cap - 1, [base + 5 * i for i in range(n)]
    assert shape == "full"
    return (cap // 2), [base + 7 * i for i in range(cap)]


# ---- what the CPU and the GPU tests share around the model ----
def window_arrays(n_groups, P, stride, cap, groups):
    """(meta u32 [P][stride], ring u64 [n_groups][P][cap]) in rg_load_inflights' form: the windows of every slot of `groups` cycle
    through the five starting shapes (group k, slot s: shape (k + s) % 5), every other window is empty -> + {(group, slot): shape}"""
    import numpy as np
    meta, ring = np.zeros((P, stride), dtype=np.uint32), np.zeros((n_groups, P, cap), dtype=np.uint64)
    shapes = {}
    for k, g in enumerate(groups):
        for s in range(P):
            shape = WINDOW_SHAPES[(k + s) % len(WINDOW_SHAPES)]
            start, entries = window_of(shape, cap, base=10 + g % 7)
            meta[s, g] = start | len(entries) << 16
            for i, e in enumerate(entries):
                ring[g, s, (start + i) % cap] = e
            shapes[(g, s)] = shape
    return meta, ring, shapes


def windows_of_group(meta, ring, cap, g, P, present):
    """The model's view of one group's windows: a list per slot with a Progress, None elsewhere"""
    out = []
    for s in range(P):
        m = int(meta[s, g])
        start, count = m & 0xFFFF, m >> 16
        out.append([int(ring[g, s, (start + i) % cap]) for i in range(count)] if present >> s & 1 else None)
    return out


def promote_state(st, meta, ring, cases, cap, **limits):
    """The model over whole arrays: the state, the window cells and the items the model expects after promoting `cases` (the refused
    ones change nothing) -> (state, meta, answers, {(group, slot): (kind, prev_index, last_index, n_msgs)}). The ring words are
    never written: an emptied window keeps its cells."""
    import handoff_rig as R
    P = st["n_slots"]
    want, want_meta, answers, items = R.copy_state(st), meta.copy(), [], {}
    for c in cases:
        m = R.get_lead(want, c.L)
        present = H.cfg_fields(m["cfg"])[4]
        win = windows_of_group(meta, ring, cap, c.L, P, present)
        a, its = promote_send(c.f, m, win, P, cap, c.persisted, **limits)
        assert a[0] == c.expect, (c.name, a)
        answers.append(a)
        if a[0] != H.DONE:
            continue
        R.put_lead(want, c.L, m)
        for s in range(P):
            if present >> s & 1:
                assert win[s] == [], (c.name, s, win[s])  # (Probe peers add nothing, the own slot never sends)
                want_meta[s, c.L] = 0
        for s, kind, prev, last, n in its:
            items[(c.L, s)] = (kind, prev, last, n)
    return want, want_meta, answers, items


N_FOLLOW, N_LEAD = 300, 130  # one full block of followed groups plus a 44-lane tail; lead groups no multiple of 64
# the configurations per slot count: (incoming, outgoing, self slot, present, transferee + 1)
CONFIGS = {
    1: [((0,), (), 0, (0,), 0)],
    3: [((0, 1, 2), (), 1, (0, 1, 2), 0), ((0, 2), (), 2, (0, 2), 0)],                       # ... and an absent slot
    5: [((0, 1, 2), (), 2, (0, 1, 2, 4), 0), ((0, 1, 2, 3, 4), (1, 3), 3, (0, 1, 2, 3, 4), 2)],  # a learner (4) beside an absent slot (3); joint with a transferee
    8: [((5, 6, 7), (4, 5, 7), 7, (1, 4, 5, 6, 7), 5), ((0, 1, 2), (), 0, (0, 1, 2, 3, 6), 0)],
}
# (log shape of handoff_model.LOG_EDGES, follow group): lanes 0-2 of one wave, both sides of a wave boundary, the last lane of the
# first block, the first and the last lane of the tail block
ROWS_BOTH = (("empty_dummy0", 0), ("one_run", 1), ("gap_present", 2), ("empty_behind_snapshot", 63), ("eight_older_plus_tail", 64), ("last_2_63_minus_2", 255),
             ("one_run", 256), ("last_2_63_minus_1", 257), ("gap_present", N_FOLLOW - 1))
LEADS = (0, N_LEAD - 1, 64, 63, 1, 77, 128, 5, 100)


def edge_cases(P, blocks="both", seed=7):
    """The promoted edges on a P-slot engine of N_LEAD groups behind an arena of N_FOLLOW: handoff_model's log shapes (one of them
    the FAULT at 2^63) x CONFIGS[P]. blocks "tail": only the rows of the arena's second block (the first block promotes nobody)."""
    import random
    rng = random.Random(seed * 100 + P)
    out = []
    for k, ((name, g), L) in enumerate(zip(ROWS_BOTH, LEADS)):
        if blocks == "tail" and g < 256:
            continue
        incoming, outgoing, self_slot, present, transferee = CONFIGS[P][k % len(CONFIGS[P])]
        cfg = H.mask(incoming) | H.mask(outgoing) << 8 | self_slot << 16 | (0x80000 if k % 3 == 2 else 0) | transferee << 20 | H.mask(present) << 24
        c, t = H.LOG_EDGES[name]
        f = H.Follower(c, t, 7, incoming, outgoing, self_slot)
        out.append(H.Case("%s_g%d" % (name, g), g, L, f, H.make_lead(P, cfg, rng, H.PF_PENDING_CONF if k % 2 else 0), c["last_index"] if k % 2 else None,
                          H.FAULT if name == "last_2_63_minus_1" else H.DONE))
    return out


def items_array(items):
    """{(group, slot): (kind, prev_index, last_index, n_msgs)} -> a SEND_ITEM_DTYPE-shaped array for sendstage.compare_items"""
    import numpy as np
    a = np.zeros(len(items), dtype=[("group", "<u8"), ("prev_index", "<u8"), ("last_index", "<u8"), ("slot", "<u4"), ("n_msgs", "<u2"), ("kind", "<u2")])
    for k, ((g, s), (kind, prev, last, n)) in enumerate(sorted(items.items())):
        a[k] = (g, prev, last, s, n, kind)
    return a


def oracle_route(st, cases, cap, max_entries=0, max_bytes=None):
    """The reference's route, all on the CPU: handoff_rig.route_state (the columns a host loads, RG_MF_BECOME_LEADER with m_hint = T),
    the oracle's tick, then its send stage over the tick's result words with the oracle's OWN Inflights (empty at the load: a
    window's starting shape is the engine's affair) -> (state after, out words, the messages sent, the cluster)."""
    import numpy as np
    import handoff_rig as R
    import oracle_lib as O
    route, msgs = R.route_state(st, cases)
    cl = O.Cluster(route["n_groups"])
    cl.load_soa(route, term=2, max_inflight=cap)
    cl.set_own_inflights(True)
    if max_bytes is not None:
        cl.set_limit_bytes(True)
        for c in cases:
            if c.expect == H.DONE:  # the one entry any message of the stage carries
                hi = c.f.canonical()["last_index"] + 1
                cl.append_entry_sizes(c.L, hi, [empty_entry_size(c.f.term, hi)])
    gout = np.zeros(route["n_groups"], dtype=np.uint32)
    cl.tick_soa(msgs, gout)
    sent = cl.send_stage_soa(gout, max_bytes if max_bytes is not None else max_entries)
    after = R.copy_state(route)
    cl.store_soa(after)
    after["run_count"] = (after["run_first"][:, :route["n_groups"]] != 0).sum(axis=0).astype(np.uint8)
    return after, gout, sent, cl
