"""The batched leader transfer (include/raftgroups_transfer.h) as a literal Python model of ONE led group:
Raft::handle_transfer_leader (src/raft.rs:1821-1889), restated line by line. Citations: pingcap/raft-rs v0.6.0.

A group is handoff_rig's dict of one group's columns (cfg, pflags, match, next, pend_rs, term_hi, dummy_index, cur_term, ...), the
windows are conf_model's (a list of P Inflights, each the list of its entries oldest first; None = an engine without device
Inflights), the send decision is conf_model.maybe_send_append -- the reference's maybe_send_append (raft.rs:773-819) called ONCE with
allow_empty = true, which is what send_append (raft.rs:760-766) is. The leader's clock cell of the group is a dict {"tag", "hb", "el"}
or None (no clock layer). csrc/rg_transfer.h is an independent restatement on values; tests/test_transfer_host.py holds the two (and
the oracle's own functions) against each other."""
import conf_model as CM

NONE, STARTED, SELF, IN_PROGRESS, LEARNER, NO_PROGRESS, NOT_LED, FAULT = range(8)
EV_TIMEOUT_NOW, EV_APPEND, EV_ABORTED_PREVIOUS = 0x1, 0x2, 0x4
TRANSFEREE_BITS = 0xF << 20
make_group, fields, window_entries, items_array = CM.make_group, CM.fields, CM.window_entries, CM.items_array


def transfer_leader(lead, windows, P, cap, t, clock=False, led=True, cell=None, max_entries=0, max_bytes=None, sizes=None, esz_w=0):
    """One selected group of rgm_transfer_leader*, t = the transferee's slot (Message.from) -> (answer dict, items [(slot, kind,
    prev_index, last_index, n_msgs)]). `lead`, `windows` and `cell` change only where the status is STARTED, or SELF with a previous
    transfer."""
    old = lead["cfg"]
    incoming, outgoing, self_slot, tr, present = fields(old)
    hi = lead["term_hi"]
    a = {"last_index": hi, "matched": lead["match"][t] if t < P and present >> t & 1 else 0, "cfg": old, "n_items": 0, "status": STARTED, "events": 0,
         "previous": 0}
    if t >= P or self_slot >= P or not present >> self_slot & 1:
        a["status"] = FAULT
    elif clock and not led:
        a["status"] = NOT_LED
    elif not present >> t & 1:  # raft.rs:1822-1829: self.prs().get(m.from).is_none()
        a["status"] = NO_PROGRESS
    elif not (incoming | outgoing) >> t & 1:  # :1832-1839: self.prs.conf().learners.contains(&from)
        a["status"] = LEARNER
    elif tr == t + 1:  # :1841-1851: the same node: ignored, election_elapsed is NOT reset
        a["status"] = IN_PROGRESS
    if a["status"] != STARTED:
        return a, []
    if tr:  # :1852 abort_leader_transfer
        lead["cfg"] = old & ~TRANSFEREE_BITS
        a.update(cfg=lead["cfg"], events=EV_ABORTED_PREVIOUS, previous=tr)
    if t == self_slot:  # :1860-1866
        a["status"] = SELF
        return a, []
    if cell is not None and cell["tag"] == lead["cur_term"]:  # :1876 election_elapsed = 0 (a cell of another term is not armed yet)
        cell["el"] = 0
    lead["cfg"] = lead["cfg"] | (t + 1) << 20  # :1877
    a["cfg"] = lead["cfg"]
    if lead["match"][t] == hi:  # :1879-1885 send_timeout_now
        a["events"] |= EV_TIMEOUT_NOW
        return a, []
    a["events"] |= EV_APPEND  # :1887 send_append = maybe_send_append(to, pr, true)
    items = []
    if windows is not None:
        m = CM.maybe_send_append(lead, windows, t, True, cap, max_entries, max_bytes, sizes, esz_w)
        if m is not None:
            items.append((t, m[0], m[1], m[2], 1))
        pb = lead["pflags"][t] & ~CM.PF_INS_FULL  # RG_PF_INS_FULL is the engine's copy of ins.full() of a Replicate peer
        lead["pflags"][t] = pb | (CM.PF_INS_FULL if (pb & CM.PF_STATE_MASK) == CM.REPLICATE and len(windows[t]) == cap else 0)
    a["n_items"] = len(items)
    return a, items


def edge_cases(P):
    """[(name, group dict, transferee slot, {slot: window shape of window_entries}, expected status)]: every status, and STARTED to a
    peer in each send state -- as far as P slots allow. A NOT_LED case wants the clock layer with the group stopped; a slot at or
    beyond P is a dense cell only (the sparse form refuses it on the host)."""
    full = (1 << P) - 1
    out = []

    def case(name, d, t, expect, windows=None):
        out.append((name, d, t, windows or {}, expect))

    if P == 1:
        case("alone_self", make_group(1, 1), 0, SELF)
        case("not_led", make_group(1, 1), 0, NOT_LED)
        case("slot_beyond", make_group(1, 1), 1, FAULT)
        d = make_group(1, 1)
        d["cfg"] &= 0x00FFFFFF  # self names a slot without a Progress
        case("self_absent", d, 0, FAULT)
        d = make_group(1, 1)
        d["cfg"] &= ~0xFF  # the only Progress is a learner's
        case("demoted_self", d, 0, LEARNER)
        case("same_again", make_group(1, 1, transferee=1), 0, IN_PROGRESS)
        return out
    a = full & ~(1 << (P - 1))  # everyone but the last slot
    # test_leader_transfer_to_uptodate_node: MsgTimeoutNow at once
    case("started_uptodate", make_group(P, full, match=[20] * P), 1, STARTED)
    # test_leader_transfer_to_slow_follower: the append first
    case("started_lagging", make_group(P, full), 1, STARTED)
    d = make_group(P, full)
    d["pflags"][1] = CM.PROBE | CM.PF_PAUSED | CM.PF_RECENT_ACTIVE
    case("started_paused_probe", d, 1, STARTED)
    d = make_group(P, full)
    d["pflags"][1] = CM.PROBE | CM.PF_RECENT_ACTIVE
    case("started_probe", d, 1, STARTED)
    d = make_group(P, full)
    d["pflags"][1] |= CM.PF_INS_FULL
    case("started_full_window", d, 1, STARTED, {1: "full"})
    d = make_group(P, full)
    d["pflags"][1] |= CM.PF_PEND_RS
    d["pend_rs"][1] = 17
    case("started_pending_request", d, 1, STARTED)
    d = make_group(P, full, dummy=12, lo=13, match=[20] * P, commit=20)
    d["pflags"][1] = CM.PROBE | CM.PF_RECENT_ACTIVE
    d["match"][1], d["next"][1] = 4, 5  # next < first_index: Compacted -> a snapshot
    case("started_compacted", d, 1, STARTED)
    d = make_group(P, full)
    d["pflags"][1] = CM.SNAPSHOT | CM.PF_RECENT_ACTIVE | CM.PF_PEND_SNAP
    d["pend_snap"][1] = 9
    case("started_snapshot_state", d, 1, STARTED)
    case("started_last_slot", make_group(P, full, self_slot=1), P - 1, STARTED)
    # test_leader_transfer_second_transfer_to_another_node / _to_same_node
    case("second_to_another", make_group(P, full, transferee=2 + 1), 1, STARTED)
    case("second_to_same", make_group(P, full, transferee=1 + 1), 1, IN_PROGRESS)
    # test_leader_transfer_to_self, with and without a transfer in progress
    case("to_self", make_group(P, full), 0, SELF)
    case("to_self_previous", make_group(P, full, transferee=1 + 1), 0, SELF)
    # test_leader_transfer_to_non_existing_node, test_leader_transfer_to_learner
    case("no_progress", make_group(P, a), P - 1, NO_PROGRESS)
    case("learner", make_group(P, a, 0, full), P - 1, LEARNER)
    # a voter of the outgoing majority alone is no learner
    case("outgoing_only", make_group(P, a, full), P - 1, STARTED)
    # a leader demoted to learner that names itself: LEARNER, not SELF
    case("demoted_self", make_group(P, full & ~1, 0, full), 0, LEARNER)
    case("not_led", make_group(P, full), 1, NOT_LED)
    case("self_absent", make_group(P, a, self_slot=P - 1), 0, FAULT)
    case("slot_beyond", make_group(P, full), P, FAULT)
    case("slot_far_beyond", make_group(P, full), 254, FAULT)
    return out


def apply_state(st, windows, recs, cap, led=None, cells=None, **limits):
    """The model over whole arrays (the SoA dicts of handoff_rig): recs = [(group, slot)]; windows = {(group, slot): [entries oldest
    first]} on an engine with device Inflights (a missing key is an empty window; updated in place) or None; led = {group: bool} where
    the leader's clock is enabled, else None; cells = {group: clock cell dict}, updated in place -> (state, answers, {(group, slot):
    (kind, prev_index, last_index, n_msgs)})"""
    import handoff_rig as R
    P = st["n_slots"]
    want, answers, items = R.copy_state(st), [], {}
    for g, t in recs:
        lead = R.get_lead(want, g)
        win = None if windows is None else [list(windows.get((g, s), [])) for s in range(P)]
        a, its = transfer_leader(lead, win, P, cap, t, clock=led is not None, led=(led or {}).get(g, True), cell=(cells or {}).get(g), **limits)
        R.put_lead(want, g, lead)
        if windows is not None:
            for s in range(P):
                windows[(g, s)] = win[s]
        answers.append(a)
        for s, kind, prev, last, n in its:
            items[(g, s)] = (kind, prev, last, n)
    return want, answers, items
