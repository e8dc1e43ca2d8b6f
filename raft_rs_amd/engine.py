"""ctypes binding of the C ABI in include/raftgroups.h (raft_rs_amd/libraftgroups.so).

Names follow the reference's domain (groups, peers/slots, progress, commit), mirroring
ProgressTracker / RaftLog accessors where one exists (citations in include/raftgroups.h).
"""
import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RG_LIB_PATH") or os.path.join(PKG, "libraftgroups.so")  # RG_LIB_PATH: tuning builds


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"raftgroups error {code}: {msg}")
        self.code = code


class COL:
    (MATCH, NEXT, PR_COMMIT, PEND_SNAP, PEND_RS, GID, PFLAGS, COMMIT, TERM_LO, TERM_HI, CFG, OUT, RUN_FIRST,
     RUN_TERM, DUMMY_INDEX, DUMMY_TERM, CUR_TERM, HOST_HINT, RUN_COUNT) = range(19)
    PER_SLOT = (0, 1, 2, 3, 4, 5)
    PER_RUN = (12, 13)
    NAMES = ("match", "next", "pr_commit", "pend_snap", "pend_rs", "gid", "pflags", "commit",
             "term_lo", "term_hi", "cfg", "out", "run_first", "run_term", "dummy_index", "dummy_term", "cur_term",
             "host_hint", "run_count")


TERM_RUNS = 8


class PF:
    STATE_MASK, PROBE, REPLICATE, SNAPSHOT, PAUSED, RECENT_ACTIVE, INS_FULL, PENDING_CONF = 0x3, 0, 1, 2, 0x4, 0x8, 0x10, 0x20


class MF:
    VALID, REJECT, HAS_RS, INS_FULL, SENT, APPEND, HEARTBEAT, HAS_LOGTERM = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
    BECOME_LEADER = 0x02  # on the leader's own slot (new term in m_hint)


class OUT:
    CHANGED, FAULT, TIMEOUT_NOW, APPENDED, BECAME_LEADER, HOST_HINT = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20

    @staticmethod
    def send_append(o):
        return (int(o) >> 8) & 0xff

    @staticmethod
    def send_more(o):
        return (int(o) >> 16) & 0xff

    @staticmethod
    def free_to(o):
        return (int(o) >> 24) & 0xff


ERR = {"NOT_ON_PATH": -9, "INVALID_ARG": -1, "NO_DEVICE": -2, "OUT_OF_MEMORY": -3, "STEP_LOCAL_MSG": -4,
       "STEP_PEER_NOT_FOUND": -5, "SLOT_BUSY": -6, "HIGHER_TERM": -7, "STATE": -8, "HOST_HINT": -10}

WL_MAJORITY, WL_JOINT, WL_MIXED = 2, 3, 5
VARIANT_DEFAULT, VARIANT_LANE, VARIANT_LDS, VARIANT_COOP, VARIANT_LDS_DMA, VARIANT_COMPACT = 0, 1, 2, 3, 4, 5


def cfg_make(incoming, outgoing=0, self_slot=0, group_commit=False, transferee_plus1=0, present=None):
    """RG_CFG_MAKE of include/raftgroups.h."""
    if present is None:
        present = incoming | outgoing
    return ((incoming & 0xff) | ((outgoing & 0xff) << 8) | ((self_slot & 7) << 16) |
            (0x00080000 if group_commit else 0) | ((transferee_plus1 & 0xf) << 20) | ((present & 0xff) << 24))


class _Config(C.Structure):
    _fields_ = [("n_groups", C.c_uint64), ("n_slots", C.c_uint32), ("device", C.c_int32),
                ("variant", C.c_uint32), ("max_inflight", C.c_uint32),
                ("cache_policy", C.c_uint32), ("flags", C.c_uint32), ("cache_resident_groups", C.c_uint64)]


class CACHE:
    """rg_config.cache_policy (include/raftgroups.h: RG_CACHE_*)."""
    AUTO, PLAIN, STREAM_MSGS, STREAM_ALL, RESIDENT = range(5)
    NAMES = ("auto", "plain", "stream_msgs", "stream_all", "resident")


class CFGF:
    """rg_config.flags (RG_CFGF_*)."""
    NO_SIZE_CLASSES, CLASS_BLOCK_ORDER, IX64, NO_READ_MIRROR = 0x1, 0x2, 0x4, 0x8


class KERNEL:
    """rg_device_info.last_tick_kernel (RG_KERNEL_*)."""
    NONE, LANE, CLASSES, SPLIT, LDS, COMPACT, TICK_SEND = range(7)
    NAMES = ("none", "k_tick_lane", "k_tick_classes", "k_tick_split", "k_tick_lds", "k_tick_compact", "k_tick_send")


HOST_HINT_DTYPE = np.dtype([("group", "<u8"), ("slot_mask", "<u4"), ("reserved", "<u4")])
RESOLVED_HINT_DTYPE = np.dtype([("group", "<u8"), ("index", "<u8"), ("hint", "<u8"), ("slot", "<u4"), ("reserved", "<u4")])
GROUP_STATUS_DTYPE = np.dtype([("group", "<u8"), ("commit", "<u8"), ("term_lo", "<u8"), ("last_index", "<u8"),
                               ("cfg", "<u4"), ("out", "<u4"), ("match", "<u8", 8), ("next", "<u8", 8),
                               ("pr_commit", "<u8", 8), ("pend_snap", "<u8", 8), ("pend_rs", "<u8", 8),
                               ("pflags", "u1", 8), ("inflights", "u1", 8)])
assert GROUP_STATUS_DTYPE.itemsize == 376


class DeviceInfo(C.Structure):
    _fields_ = [("arch", C.c_char * 32), ("compute_units", C.c_uint32), ("wavefront", C.c_uint32),
                ("lds_per_workgroup", C.c_uint64), ("hbm_bytes", C.c_uint64), ("l2_bytes", C.c_uint64),
                ("engine_bytes", C.c_uint64), ("cache_policy", C.c_uint32), ("engines_on_device", C.c_uint32),
                ("resident_groups", C.c_uint64), ("last_tick_kernel", C.c_uint32), ("last_tick_streaming", C.c_uint32),
                ("infinity_cache_bytes", C.c_uint64), ("infinity_cache_queried", C.c_uint32), ("last_tick_offset_bits", C.c_uint32)]


import contextlib


@contextlib.contextmanager
def config_defaults(**kw):
    """Every Engine created inside the block gets these rg_config fields unless it names them itself."""
    old = dict(Engine._defaults)
    Engine._defaults.update(kw)
    try:
        yield
    finally:
        Engine._defaults.clear()
        Engine._defaults.update(old)


class _Msgs(C.Structure):
    _fields_ = [("m_index", C.c_void_p), ("m_commit", C.c_void_p), ("m_hint", C.c_void_p),
                ("m_rs", C.c_void_p), ("m_flags", C.c_void_p), ("m_logterm", C.c_void_p)]


class _Workload(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("workload", C.c_uint32), ("reserved", C.c_uint32)]


class _HostState(C.Structure):
    _fields_ = [("n_groups", C.c_uint64), ("stride", C.c_uint64), ("n_slots", C.c_uint32),
                ("reserved", C.c_uint32)] + \
               [(n, C.c_void_p) for n in ("match", "next", "pr_commit", "pend_snap", "pend_rs", "gid",
                                          "pflags", "commit", "term_lo", "term_hi", "cfg")]


class AppendResponse(C.Structure):
    _fields_ = [("from_", C.c_uint64), ("term", C.c_uint64), ("index", C.c_uint64), ("commit", C.c_uint64),
                ("reject_hint", C.c_uint64), ("request_snapshot", C.c_uint64), ("reject", C.c_uint8),
                ("ins_full", C.c_uint8), ("pad", C.c_uint8 * 6), ("log_term", C.c_uint64)]


class DecodedMessage(C.Structure):
    """rg_decoded_message: the fields of one protobuf-encoded eraftpb::Message (rg_decode_message)."""
    _fields_ = [("msg_type", C.c_uint32), ("reject", C.c_uint32), ("to", C.c_uint64), ("from_", C.c_uint64),
                ("term", C.c_uint64), ("log_term", C.c_uint64), ("index", C.c_uint64), ("commit", C.c_uint64),
                ("commit_term", C.c_uint64), ("reject_hint", C.c_uint64), ("request_snapshot", C.c_uint64),
                ("priority", C.c_uint64), ("n_entries", C.c_uint64), ("has_snapshot", C.c_uint32),
                ("context_len", C.c_uint32)]


class EntryC(C.Structure):
    """rg_entry: one eraftpb::Entry handed to the encoder (rg_entry_size / rg_limit_size / rg_encode_message)."""
    _fields_ = [("entry_type", C.c_uint32), ("sync_log", C.c_uint32), ("term", C.c_uint64), ("index", C.c_uint64),
                ("data", C.c_char_p), ("data_len", C.c_uint64), ("context", C.c_char_p), ("context_len", C.c_uint64)]


class MessageC(C.Structure):
    """rg_message: an outgoing eraftpb::Message (rg_message_size / rg_encode_message)."""
    _fields_ = [("msg_type", C.c_uint32), ("reject", C.c_uint32), ("to", C.c_uint64), ("from_", C.c_uint64),
                ("term", C.c_uint64), ("log_term", C.c_uint64), ("index", C.c_uint64), ("commit", C.c_uint64),
                ("commit_term", C.c_uint64), ("reject_hint", C.c_uint64), ("request_snapshot", C.c_uint64),
                ("priority", C.c_uint64), ("entries", C.POINTER(EntryC)), ("n_entries", C.c_uint64),
                ("snapshot", C.c_char_p), ("snapshot_len", C.c_uint64), ("context", C.c_char_p), ("context_len", C.c_uint64)]


class WireMsg(C.Structure):
    _fields_ = [("group", C.c_uint64), ("index", C.c_uint64), ("commit", C.c_uint64), ("hint", C.c_uint64),
                ("rs", C.c_uint64), ("log_term", C.c_uint64), ("slot", C.c_uint32), ("flags", C.c_uint32),
                ("pad", C.c_uint64)]


WIRE_DTYPE = np.dtype([("group", "<u8"), ("index", "<u8"), ("commit", "<u8"), ("hint", "<u8"), ("rs", "<u8"),
                       ("log_term", "<u8"), ("slot", "<u4"), ("flags", "<u4"), ("pad", "<u8")])
assert WIRE_DTYPE.itemsize == 64


class CellWrite(C.Structure):
    _fields_ = [("group", C.c_uint64), ("slot", C.c_uint32), ("field_mask", C.c_uint32),
                ("match", C.c_uint64), ("next", C.c_uint64), ("pr_commit", C.c_uint64),
                ("pend_snap", C.c_uint64), ("pend_rs", C.c_uint64), ("gid", C.c_uint64),
                ("pflags", C.c_uint8), ("pad", C.c_uint8 * 7)]


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)


class CommConfig(C.Structure):
    _fields_ = [("rank", C.c_uint32), ("world", C.c_uint32), ("unique_id", C.c_void_p), ("transport", ALLGATHER_FN),
                ("transport_user", C.c_void_p), ("ring_ticks", C.c_uint32), ("overflow_slots", C.c_uint32)]


class PublishStats(C.Structure):
    _fields_ = [("publications", C.c_uint64), ("full_publications", C.c_uint64), ("replica_updates", C.c_uint64),
                ("bytes_per_rank_last", C.c_uint64), ("bytes_per_rank_delta", C.c_uint64),
                ("bytes_per_rank_full", C.c_uint64), ("overflow_slots", C.c_uint32), ("ring_ticks", C.c_uint32),
                ("host_us_events", C.c_double), ("host_us_allgather", C.c_double), ("host_us_memset", C.c_double),
                ("events_on_tick_packets", C.c_uint64)]


ABI_VERSION = 12  # RG_ABI_VERSION of include/raftgroups.h these ctypes layouts mirror (tests/test_abi.py compares)
class CommInfo(C.Structure):
    _fields_ = [("rank", C.c_uint32), ("world", C.c_uint32), ("transport", C.c_uint32), ("in_process", C.c_uint32),
                ("rccl_ranks", C.c_uint32), ("rccl_rank", C.c_uint32)]


TRANSPORT_NAMES = {0: "none", 1: "rccl", 2: "callback", 3: "local"}
COMM_ID_BYTES = 128
PUBLISH_FULL = 1

SEND_APPEND, SEND_SNAPSHOT, SEND_HOST = 1, 2, 3
SEND_SKIP_BCAST_COMMIT = 1
SEND_BYTES = 2
NO_LIMIT = (1 << 64) - 1
LOG_SIZE_DTYPE = np.dtype([("group", "<u8"), ("index", "<u8"), ("cum_bytes", "<u8")])
SENT_MSG_DTYPE = np.dtype([("group", "<u8"), ("last", "<u8"), ("slot", "<u4"), ("reserved", "<u4")])
PROGRESS_EVENT_DTYPE = np.dtype([("group", "<u8"), ("slot", "<u4"), ("kind", "<u4")])  # rg_progress_event
EV_UNREACHABLE, EV_SNAPSHOT_FINISH, EV_SNAPSHOT_FAILURE = 1, 2, 3
SEND_ITEM_DTYPE = np.dtype([("group", "<u8"), ("prev_index", "<u8"), ("last_index", "<u8"), ("slot", "<u4"),
                            ("n_msgs", "<u2"), ("kind", "<u2")])
assert SEND_ITEM_DTYPE.itemsize == 32
# ReadIndex (rg_read_index_enable ...)
READ_REQ_DTYPE = np.dtype([("group", "<u8"), ("ctx", "<u8")])                                     # rg_read_req
READ_ACK_DTYPE = np.dtype([("group", "<u8"), ("ctx", "<u8"), ("slot", "<u4"), ("flags", "<u4")])  # rg_read_ack
READ_STATE_DTYPE = np.dtype([("group", "<u8"), ("ctx", "<u8"), ("index", "<u8")])                 # rg_read_state
READ_LEASE = 1
READ_ACK_LAST_SELF = 1
READ_NOT_READY, READ_READY, READ_QUEUED, READ_DUPLICATE, READ_FULL = 0, 1, 2, 3, 4
READ_MAX_DEPTH = 16
# The follower half (rg_follow_enable ...)
FOLLOW_RUNS = 9
FOLLOW_STATE_DTYPE = np.dtype([("group", "<u8"), ("committed", "<u8"), ("last_index", "<u8"), ("dummy_index", "<u8"), ("dummy_term", "<u8"),
                               ("n_runs", "<u4"), ("reserved", "<u4"), ("run_first", "<u8", (FOLLOW_RUNS,)),
                               ("run_term", "<u8", (FOLLOW_RUNS,))])                                # rg_follow_state
FOLLOW_ENT_RUN_DTYPE = np.dtype([("term", "<u8"), ("count", "<u4"), ("reserved", "<u4")])           # rg_follow_ent_run
FOLLOW_MSG_DTYPE = np.dtype([("group", "<u8"), ("index", "<u8"), ("log_term", "<u8"), ("commit", "<u8"), ("ent_term", "<u8"),
                             ("n_entries", "<u4"), ("flags", "<u4"), ("ext", "<u8")])               # rg_follow_msg
FOLLOW_RESP_DTYPE = np.dtype([("index", "<u8"), ("commit", "<u8"), ("conflict", "<u8"), ("reject_hint", "<u8"), ("log_term", "<u8"),
                              ("status", "<u4"), ("reserved", "<u4")])                              # rg_follow_resp
assert (FOLLOW_STATE_DTYPE.itemsize, FOLLOW_ENT_RUN_DTYPE.itemsize, FOLLOW_MSG_DTYPE.itemsize, FOLLOW_RESP_DTYPE.itemsize) == (192, 16, 56, 48)
FOLLOW_MSG_APPEND, FOLLOW_MSG_HEARTBEAT = 1, 2
FOLLOW_NONE, FOLLOW_ACCEPT, FOLLOW_REJECT, FOLLOW_STALE, FOLLOW_HEARTBEAT, FOLLOW_FAULT, FOLLOW_HOST = 0, 1, 2, 3, 4, 5, 6
# ... its term gate, vote step and election clock (rg_follow_gate_enable ...)
FOLLOW_SOFT_DTYPE = np.dtype([("group", "<u8"), ("term", "<u8"), ("vote", "<u8"), ("leader_id", "<u8"), ("priority", "<i8"),
                              ("election_elapsed", "<u4"), ("randomized_timeout", "<u4"), ("role", "u1"), ("promotable", "u1"),
                              ("reserved", "u1", (6,))])                                             # rg_follow_soft
FOLLOW_HDR_DTYPE = np.dtype([("term", "<u8"), ("from", "<u8"), ("priority", "<i8"), ("flags", "<u4"), ("reserved", "<u4")])  # rg_follow_hdr
FOLLOW_GATE_RESP_DTYPE = np.dtype([("term", "<u8"), ("gate", "<u4"), ("events", "<u4")])            # rg_follow_gate_resp
assert (FOLLOW_SOFT_DTYPE.itemsize, FOLLOW_HDR_DTYPE.itemsize, FOLLOW_GATE_RESP_DTYPE.itemsize) == (56, 32, 16)
FOLLOW_MSG_VOTE, FOLLOW_MSG_PREVOTE, FOLLOW_MSG_TOUCH = 4, 8, 16
GATE_CHECK_QUORUM, GATE_PRE_VOTE = 1, 2
GATE_FORCE = 1
GATE_NONE, GATE_PASS, GATE_IGNORED, GATE_STALE_LEADER, GATE_PREVOTE_LOW, GATE_VOTE_GRANT, GATE_VOTE_REJECT = 0, 1, 2, 3, 4, 5, 6
GATE_EV_HARD_STATE, GATE_EV_BECAME_FOLLOWER, GATE_EV_LEADER_CHANGED, GATE_EV_CONF_CHECK = 1, 2, 4, 8
ROLE_FOLLOWER, ROLE_PRE_CANDIDATE, ROLE_CANDIDATE = 0, 1, 2
# ... and the candidate half: campaign, vote responses and poll (rg_follow_elect_enable ...)
FOLLOW_ELECT_DTYPE = np.dtype([("group", "<u8"), ("self_id", "<u8"), ("conf", "<u4"), ("yes", "u1"), ("no", "u1"), ("reserved", "u1", (2,))])  # rg_follow_elect
FOLLOW_ELECT_RESP_DTYPE = np.dtype([("term", "<u8"), ("req_term", "<u8"), ("req_index", "<u8"), ("req_log_term", "<u8"), ("req_commit", "<u8"),
                                    ("req_commit_term", "<u8"), ("result", "<u4"), ("events", "<u4"), ("req_kind", "<u4"), ("targets", "<u4"),
                                    ("status", "<u4"), ("flags", "<u4")])                           # rg_follow_elect_resp
FOLLOW_CAMPAIGN_REQ_DTYPE = np.dtype([("group", "<u8"), ("term", "<u8"), ("from", "<u8"), ("flags", "<u4"), ("reserved", "<u4")])  # rg_follow_campaign_req
FOLLOW_VOTE_REC_DTYPE = np.dtype([("group", "<u8"), ("term", "<u8"), ("commit", "<u8"), ("commit_term", "<u8"), ("from_slot", "u1"), ("kind", "u1"),
                                  ("reject", "u1"), ("reserved", "u1", (5,))])                       # rg_follow_vote_rec
assert (FOLLOW_ELECT_DTYPE.itemsize, FOLLOW_ELECT_RESP_DTYPE.itemsize, FOLLOW_CAMPAIGN_REQ_DTYPE.itemsize, FOLLOW_VOTE_REC_DTYPE.itemsize) == (24, 72, 32, 40)
ELECT_NONE, ELECT_IGNORED, ELECT_BLOCKED, ELECT_REQUESTS, ELECT_PENDING, ELECT_LOST, ELECT_WON, ELECT_STEPPED_DOWN = range(8)
ELECT_REQ_TRANSFER = 1
CAMPAIGN_TIMEOUT_NOW, CAMPAIGN_BLOCKED = 1, 2
ELECT_OUT_COLUMNS = ("result", "events", "status", "req_kind", "targets", "flags", "term", "req_term", "req_index", "req_log_term", "req_commit",
                     "req_commit_term")  # rg_follow_elect_out: six u8 columns, six u64 columns
VOTE_COLUMNS = ("kind", "slot", "reject", "term", "commit", "commit_term")  # rg_follow_vote_cols: three u8 columns, three u64 columns
# ... and the hand-off between the arena and the leader columns (rg_follow_promote / rg_follow_demote ...)
HANDOFF_REC_DTYPE = np.dtype([("follow_group", "<u8"), ("lead_group", "<u8"), ("persisted", "<u8")])                              # rg_handoff_rec
HANDOFF_RESP_DTYPE = np.dtype([("term", "<u8"), ("last_index", "<u8"), ("commit", "<u8"), ("status", "<u4"), ("out", "<u4")])  # rg_handoff_resp
assert (HANDOFF_REC_DTYPE.itemsize, HANDOFF_RESP_DTYPE.itemsize) == (24, 32)
HANDOFF_NONE, HANDOFF_DONE, HANDOFF_NOT_WON, HANDOFF_CONF, HANDOFF_NOT_PERSISTED, HANDOFF_FAULT = range(6)
HANDOFF_OUT_COLUMNS = ("status", "term", "last_index")  # rg_handoff_out: one u8 column, two u64 columns
LEAD_VERSION = 1  # RGX_LEAD_VERSION of include/raftgroups_lead.h the leader-clock layouts below mirror
HANDOFF_NO_LEAD = 0xFFFFFFFFFFFFFFFF  # RG_HANDOFF_NO_LEAD: a dev_lead cell of follow_step_down_device that names no lead group
# ... and the leader's clock (rgx_lead_clock_enable ...)
LEAD_CLOCK_CELL_DTYPE = np.dtype([("group", "<u8"), ("term", "<u8"), ("election_elapsed", "<u4"), ("heartbeat_elapsed", "<u4"),
                                  ("led", "u1"), ("reserved", "u1", (7,))])  # rg_lead_clock_cell
assert LEAD_CLOCK_CELL_DTYPE.itemsize == 32
LEAD_CLOCK_START_LED = 0x100
LEAD_EV_BEAT, LEAD_EV_CHECK_QUORUM, LEAD_EV_STEPPED_DOWN, LEAD_EV_TRANSFER_ABORTED, LEAD_EV_NEW_TERM = 0x1, 0x2, 0x4, 0x8, 0x10
LEAD_CLOCK_OUT_FIELDS = ("events", "beat", "beat_cap", "down", "down_cap", "hb_commit")  # rg_lead_clock_out
# ... and the leader's term gate and the deposition (include/raftgroups_term.h: rgt_lead_gate_device ...)
TERM_VERSION = 1  # RGT_TERM_VERSION
TERM_GATE_EV_TRANSFER_ABORTED, TERM_GATE_EV_STALE, TERM_GATE_EV_NOT_LED, TERM_GATE_EV_DEPOSED = 0x08, 0x20, 0x40, 0x80
TERM_GATE_OUT_FIELDS = ("flags", "events", "new_term", "down", "down_cap")  # rgt_lead_gate_out
DEPOSE_REC_DTYPE = np.dtype([("follow_group", "<u8"), ("lead_group", "<u8"), ("term", "<u8"), ("reserved", "<u8")])  # rgt_depose_rec
assert DEPOSE_REC_DTYPE.itemsize == 32
# ... and the dense vote step (include/raftgroups_vote.h: rgv_follow_vote_device ...)
VOTE_VERSION = 1  # RGV_VOTE_VERSION
VOTE_EV_LED, VOTE_EV_TRANSFER_ABORTED, VOTE_EV_DEPOSED = 0x20, 0x40, 0x80
VOTE_OUT_FIELDS = ("status", "gate", "events", "term", "commit", "log_term", "answered", "answered_cap")  # rgv_vote_out
VOTE_REC_DTYPE = np.dtype([("follow_group", "<u8"), ("lead_group", "<u8"), ("term", "<u8"), ("from", "<u8"), ("index", "<u8"), ("log_term", "<u8"),
                           ("commit", "<u8"), ("commit_term", "<u8"), ("priority", "<i8"), ("kind", "<u4"), ("flags", "<u4")])  # rgv_vote_rec
VOTE_RESP_DTYPE = np.dtype([("term", "<u8"), ("commit", "<u8"), ("log_term", "<u8"), ("last_index", "<u8"), ("gate", "<u4"), ("events", "<u4"),
                            ("status", "<u4"), ("reserved", "<u4")])  # rgv_vote_resp
assert VOTE_REC_DTYPE.itemsize == 80 and VOTE_RESP_DTYPE.itemsize == 48
# ... and the promotion into an engine with device Inflights (include/raftgroups_handoff.h: rgh_follow_promote ...)
HANDOFF_EXT_VERSION = 1  # RGH_HANDOFF_VERSION
PROMOTE_OUT_FIELDS = ("out", "items", "item_cap", "count")  # rgh_promote_out
# ... and the batched conf change (include/raftgroups_conf.h: rgc_apply_conf ...)
CONF_VERSION = 1  # RGC_CONF_VERSION
CONF_NONE, CONF_DONE, CONF_DEMOTED, CONF_NOT_LED, CONF_HOST, CONF_FAULT = 0, 1, 2, 3, 4, 5
CONF_EV_COMMITTED, CONF_EV_TRANSFER_ABORTED = 0x1, 0x2
CONF_REC_DTYPE = np.dtype([("group", "<u8"), ("cfg", "<u4"), ("reserved", "<u4")])  # rgc_conf_rec
CONF_RESP_DTYPE = np.dtype([("commit", "<u8"), ("last_index", "<u8"), ("cfg", "<u4"), ("out", "<u4"), ("n_items", "<u4"), ("status", "u1"),
                            ("events", "u1"), ("added", "u1"), ("removed", "u1")])  # rgc_conf_resp
assert CONF_REC_DTYPE.itemsize == 16 and CONF_RESP_DTYPE.itemsize == 32
CONF_OUT_FIELDS = ("status", "events", "commit", "items", "item_cap", "count")  # rgc_conf_out
# ... and the batched leader transfer (include/raftgroups_transfer.h: rgm_transfer_leader ...)
TRANSFER_VERSION = 1  # RGM_TRANSFER_VERSION
MIRROR_VERSION = 1  # RGR_MIRROR_VERSION (include/raftgroups_mirror.h)
XFER_NONE, XFER_STARTED, XFER_SELF, XFER_IN_PROGRESS, XFER_LEARNER, XFER_NO_PROGRESS, XFER_NOT_LED, XFER_FAULT = range(8)
XFER_EV_TIMEOUT_NOW, XFER_EV_APPEND, XFER_EV_ABORTED_PREVIOUS = 0x1, 0x2, 0x4
TRANSFER_REC_DTYPE = np.dtype([("group", "<u8"), ("slot", "<u4"), ("reserved", "<u4")])  # rgm_transfer_rec
TRANSFER_RESP_DTYPE = np.dtype([("last_index", "<u8"), ("matched", "<u8"), ("cfg", "<u4"), ("n_items", "<u4"), ("status", "u1"), ("events", "u1"),
                                ("previous", "u1"), ("reserved", "u1"), ("reserved2", "<u4")])  # rgm_transfer_resp
assert TRANSFER_REC_DTYPE.itemsize == 16 and TRANSFER_RESP_DTYPE.itemsize == 32
TRANSFER_OUT_FIELDS = ("status", "events", "items", "item_cap", "count")  # rgm_transfer_out


def elect_conf_make(incoming, outgoing=0, self_slot=0):
    """RG_ELECT_CONF_MAKE"""
    return (incoming & 0xFF) | ((outgoing & 0xFF) << 8) | ((self_slot & 7) << 16)


class FollowGateConfig(C.Structure):  # rg_follow_gate_config
    _fields_ = [("election_tick", C.c_uint32), ("min_timeout", C.c_uint32), ("max_timeout", C.c_uint32), ("flags", C.c_uint32),
                ("seed", C.c_uint64)]


class FollowMsgs(C.Structure):  # rg_follow_msgs: device pointers
    _fields_ = [("flags", C.c_void_p), ("index", C.c_void_p), ("log_term", C.c_void_p), ("commit", C.c_void_p), ("ent_term", C.c_void_p),
                ("n_entries", C.c_void_p), ("ext", C.c_void_p), ("ext_runs", C.c_void_p), ("n_ext", C.c_uint64)]


class FollowOut(C.Structure):  # rg_follow_out: device pointers
    _fields_ = [("status", C.c_void_p), ("index", C.c_void_p), ("commit", C.c_void_p), ("conflict", C.c_void_p),
                ("reject_hint", C.c_void_p), ("log_term", C.c_void_p)]


class FollowElectOut(C.Structure):  # rg_follow_elect_out: device pointers
    _fields_ = [(k, C.c_void_p) for k in ELECT_OUT_COLUMNS]


class FollowVoteCols(C.Structure):  # rg_follow_vote_cols: device pointers
    _fields_ = [(k, C.c_void_p) for k in VOTE_COLUMNS]


class HandoffOut(C.Structure):  # rg_handoff_out: device pointers
    _fields_ = [(k, C.c_void_p) for k in HANDOFF_OUT_COLUMNS]


class LeadClockConfig(C.Structure):  # rg_lead_clock_config
    _fields_ = [("election_tick", C.c_uint32), ("heartbeat_tick", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class LeadClockOut(C.Structure):  # rg_lead_clock_out: device pointers and the two list capacities
    _fields_ = [(k, C.c_uint64 if k.endswith("_cap") else C.c_void_p) for k in LEAD_CLOCK_OUT_FIELDS]


class TermGateOut(C.Structure):  # rgt_lead_gate_out: device pointers and the list capacity
    _fields_ = [(k, C.c_uint64 if k.endswith("_cap") else C.c_void_p) for k in TERM_GATE_OUT_FIELDS]


class VoteOut(C.Structure):  # rgv_vote_out: device pointers and the list capacity
    _fields_ = [(k, C.c_uint64 if k.endswith("_cap") else C.c_void_p) for k in VOTE_OUT_FIELDS]


class PromoteOut(C.Structure):  # rgh_promote_out: the answer columns, the caller's item list and its count word, all DEVICE memory
    _fields_ = [("out", HandoffOut), ("items", C.c_void_p), ("item_cap", C.c_uint64), ("count", C.c_void_p)]


class ConfOut(C.Structure):  # rgc_conf_out: the answer columns, the caller's item list and its count word, all DEVICE memory
    _fields_ = [(k, C.c_uint64 if k.endswith("_cap") else C.c_void_p) for k in CONF_OUT_FIELDS]


class MirrorInfo(C.Structure):  # rgr_mirror_info (include/raftgroups_mirror.h): the dense tick's read mirror, host-side counters
    _fields_ = [("packed_launches", C.c_uint64), ("build_launches", C.c_uint64), ("plane_bytes", C.c_uint64), ("present", C.c_uint32),
                ("valid", C.c_uint32), ("off", C.c_uint32), ("version", C.c_uint32)]


class TransferOut(C.Structure):  # rgm_transfer_out: the answer columns, the caller's item list and its count word, all DEVICE memory
    _fields_ = [(k, C.c_uint64 if k.endswith("_cap") else C.c_void_p) for k in TRANSFER_OUT_FIELDS]


# every symbol include/raftgroups.h declares: (restype, argtypes)
_vp, _u64, _i = C.c_void_p, C.c_uint64, C.c_int
SYMBOLS = {
    "rg_version": (C.c_char_p, []),
    "rg_abi_version": (C.c_uint32, []),
    "rg_last_error": (C.c_char_p, []),
    "rg_device_count": (_i, []),
    "rg_create": (_i, [C.POINTER(_Config), C.POINTER(_vp)]),
    "rg_destroy": (None, [_vp]),
    "rg_stride": (_u64, [_vp]),
    "rg_get_device_info": (_i, [_vp, C.POINTER(DeviceInfo)]),
    "rg_set_stream": (_i, [_vp, _vp]),
    "rg_sync": (_i, [_vp]),
    "rg_column_bytes": (_u64, [_vp, _i]),
    "rg_load_column": (_i, [_vp, _i, _vp, _u64]),
    "rg_read_column": (_i, [_vp, _i, _vp, _u64]),
    "rg_column_ptr": (_vp, [_vp, _i]),
    "rg_checkpoint": (_i, [_vp]),
    "rg_restore": (_i, [_vp]),
    "rg_read_groups": (_i, [_vp, _vp, _u64, _vp]),
    "rg_write_cells": (_i, [_vp, C.POINTER(CellWrite), _u64]),
    "rg_set_config": (_i, [_vp, _u64, C.c_uint32]),
    "rg_tick": (_i, [_vp, C.POINTER(_Msgs)]),
    "rg_tick_device": (_i, [_vp, C.POINTER(_Msgs)]),
    "rg_tick_device_fused": (_i, [_vp, C.POINTER(_Msgs), C.c_uint32, _vp, _vp]),
    "rg_fused_ticks_done": (_i, [_vp, C.POINTER(C.c_uint32)]),
    "rg_recompute": (_i, [_vp]),
    "rg_maximal_committed_index": (_i, [_vp, _vp, _vp]),
    "rg_results": (_i, [_vp, _vp, _vp]),
    "rg_heartbeat_commits": (_i, [_vp, _vp, _vp]),
    "rg_step_heartbeat_response": (_i, [_vp, _u64, _u64, _u64, _u64, C.c_uint8]),
    "rg_result_counts": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "rg_plan_placement": (_i, [_vp, _u64, C.c_uint32, _vp, _vp, C.c_uint32, C.POINTER(C.c_uint32)]),
    "rg_permute_groups": (_i, [_vp, _vp]),
    "rg_size_classes": (_i, [_vp, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "rg_host_hints": (_i, [_vp, C.c_void_p, _u64, C.POINTER(_u64)]),
    "rg_resolve_host_hints": (_i, [_vp, C.c_void_p, _u64, C.c_void_p]),
    "rg_msg_stats": (_i, [_vp, _vp, C.POINTER(_u64 * 5)]),
    "rg_ingest": (_i, [_vp, _vp, _u64, C.POINTER(_u64)]),
    "rg_ingest_device": (_i, [_vp, _vp, _u64]),
    "rg_ingested_duplicates": (_i, [_vp, C.POINTER(_u64)]),
    "rg_tick_ingested": (_i, [_vp, C.POINTER(_u64)]),
    "rg_ingest_tick": (_i, [_vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "rg_ingested_results": (_i, [_vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    "rg_send_appends": (_i, [_vp, _u64, C.c_uint32]),
    "rg_tick_send": (_i, [_vp, _vp, _u64, C.c_uint32]),
    "rg_tick_device_send": (_i, [_vp, _vp, _u64, C.c_uint32]),
    "rg_flush_send": (_i, [_vp, _u64, C.c_uint32]),
    "rg_mailbox_start": (_i, [_vp, C.c_uint32]),
    "rg_mailbox_stop": (_i, [_vp]),
    "rg_mailbox_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "rg_log_sizes_enable": (_i, [_vp, C.c_uint32]),
    "rg_log_sizes_write": (_i, [_vp, _vp, _u64]),
    "rg_workload_sizes": (_i, [_vp, _u64, C.c_uint32, C.c_uint32]),
    "rg_update_state": (_i, [_vp, _vp, _u64]),
    "rg_send_items": (_i, [_vp, _vp, _u64, C.POINTER(_u64)]),
    "rg_send_items_ptr": (_vp, [_vp]),
    "rg_send_columns": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "rg_send_tail_column": (_i, [_vp, C.POINTER(_vp)]),
    "rg_inflights_bytes": (_u64, [_vp, _i]),
    "rg_read_inflights": (_i, [_vp, _vp, _vp]),
    "rg_load_inflights": (_i, [_vp, _vp, _vp]),
    "rg_vote_result": (_i, [_vp, _vp, _vp, _vp]),
    "rg_tally_votes": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "rg_quorum_recently_active": (_i, [_vp, _vp]),
    "rg_read_index_enable": (_i, [_vp, C.c_uint32]),
    "rg_read_index": (_i, [_vp, _vp, _u64, C.c_uint32, _vp]),
    "rg_read_acks": (_i, [_vp, _vp, _u64]),
    "rg_read_acks_device": (_i, [_vp, _vp]),
    "rg_read_states": (_i, [_vp, _vp, _u64, C.POINTER(_u64)]),
    "rg_read_last_pending": (_i, [_vp, _vp, _vp]),
    "rg_read_pending_counts": (_i, [_vp, _vp]),
    "rg_follow_enable": (_i, [_vp, _u64]),
    "rg_follow_stride": (_u64, [_vp]),
    "rg_follow_write": (_i, [_vp, _vp, _u64]),
    "rg_follow_read": (_i, [_vp, _vp, _u64, _vp]),
    "rg_follow_step": (_i, [_vp, _vp, _u64, _vp, _u64, _vp]),
    "rg_follow_step_device": (_i, [_vp, C.POINTER(FollowMsgs), C.POINTER(FollowOut)]),
    "rg_follow_gate_enable": (_i, [_vp, C.POINTER(FollowGateConfig)]),
    "rg_follow_soft_write": (_i, [_vp, _vp, _u64]),
    "rg_follow_soft_read": (_i, [_vp, _vp, _u64, _vp]),
    "rg_follow_step_gated": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp]),
    "rg_follow_step_gated_device": (_i, [_vp, C.POINTER(FollowMsgs), _vp, _vp, C.POINTER(FollowOut), _vp, _vp, _vp]),
    "rg_follow_clock": (_i, [_vp, _vp, _u64, _vp]),
    "rg_follow_clock_counts": (_vp, [_vp]),
    "rg_follow_elect_enable": (_i, [_vp]),
    "rg_follow_elect_write": (_i, [_vp, _vp, _u64]),
    "rg_follow_elect_read": (_i, [_vp, _vp, _u64, _vp]),
    "rg_follow_campaign_device": (_i, [_vp, _vp, _vp, _u64, _vp, C.POINTER(FollowElectOut)]),
    "rg_follow_campaign": (_i, [_vp, _vp, _u64, _vp]),
    "rg_follow_vote_resps": (_i, [_vp, _vp, _u64, _vp]),
    "rg_follow_vote_resps_device": (_i, [_vp, C.POINTER(FollowVoteCols), C.POINTER(FollowElectOut)]),
    "rg_follow_promote": (_i, [_vp, _vp, _u64, _vp]),
    "rg_follow_promote_device": (_i, [_vp, _vp, _vp, _vp, C.POINTER(HandoffOut)]),
    "rg_follow_demote": (_i, [_vp, _vp, _u64, _vp]),
    "rg_follow_demote_device": (_i, [_vp, _vp, _vp, C.POINTER(HandoffOut)]),
    "rgx_lead_version": (C.c_uint32, []),
    "rgx_lead_clock_enable": (_i, [_vp, C.POINTER(LeadClockConfig)]),
    "rgx_lead_clock_write": (_i, [_vp, _vp, _u64]),
    "rgx_lead_clock_read": (_i, [_vp, _vp, _u64, _vp]),
    "rgx_lead_clock": (_i, [_vp, C.POINTER(LeadClockOut), _vp]),
    "rgx_lead_clock_counts": (_vp, [_vp]),
    "rgx_follow_step_down": (_i, [_vp, _vp, _u64, _vp]),
    "rgx_follow_step_down_device": (_i, [_vp, _vp, _vp, C.POINTER(HandoffOut)]),
    "rgt_term_version": (C.c_uint32, []),
    "rgt_lead_gate_device": (_i, [_vp, C.POINTER(_Msgs), _vp, C.POINTER(TermGateOut), _vp]),
    "rgt_lead_gate_counts": (_vp, [_vp]),
    "rgt_follow_depose": (_i, [_vp, _vp, _u64, _vp]),
    "rgt_follow_depose_device": (_i, [_vp, _vp, _vp, _vp, C.POINTER(HandoffOut)]),
    "rgt_follow_depose_scan_device": (_i, [_vp, _vp, _vp, _vp, C.POINTER(HandoffOut)]),
    "rgv_vote_version": (C.c_uint32, []),
    "rgv_follow_vote_device": (_i, [_vp, C.POINTER(FollowMsgs), _vp, _vp, _vp, _vp, _vp, C.POINTER(VoteOut), _vp]),
    "rgv_follow_vote": (_i, [_vp, _vp, _u64, _vp]),
    "rgv_follow_vote_counts": (_vp, [_vp]),
    "rgh_handoff_version": (C.c_uint32, []),
    "rgh_follow_promote": (_i, [_vp, _vp, _u64, _vp, _u64, C.c_uint32, _vp, _u64, C.POINTER(_u64)]),
    "rgh_follow_promote_device": (_i, [_vp, _vp, _vp, _vp, _u64, C.c_uint32, C.POINTER(PromoteOut)]),
    "rgc_conf_version": (C.c_uint32, []),
    "rgc_apply_conf": (_i, [_vp, _vp, _u64, _vp, _u64, C.c_uint32, _vp, _u64, C.POINTER(_u64)]),
    "rgc_apply_conf_device": (_i, [_vp, _vp, _vp, _u64, C.c_uint32, C.POINTER(ConfOut)]),
    "rgm_transfer_version": (C.c_uint32, []),
    "rgm_transfer_leader": (_i, [_vp, _vp, _u64, _vp, _u64, C.c_uint32, _vp, _u64, C.POINTER(_u64)]),
    "rgm_transfer_leader_device": (_i, [_vp, _vp, _u64, C.c_uint32, C.POINTER(TransferOut)]),
    "rg_set_peers": (_i, [_vp, _u64, C.POINTER(_u64), C.c_uint32, _u64]),
    "rg_step": (_i, [_vp, _u64, C.POINTER(AppendResponse)]),
    "rg_step_bytes": (_i, [_vp, _u64, C.c_char_p, _u64, C.c_uint8]),
    "rg_decode_message": (_i, [C.c_char_p, _u64, C.POINTER(DecodedMessage)]),
    "rg_progress_events": (_i, [_vp, C.c_void_p, _u64]),
    "rg_progress_event_dense": (_i, [_vp, C.c_uint32, C.c_void_p]),
    "rg_report_unreachable": (_i, [_vp, _u64, _u64]),
    "rg_report_snapshot": (_i, [_vp, _u64, _u64, _i]),
    "rg_entry_size": (_u64, [C.POINTER(EntryC)]),
    "rg_limit_size": (_u64, [C.POINTER(EntryC), _u64, _u64]),
    "rg_message_size": (_i, [C.POINTER(MessageC), C.POINTER(C.c_uint64)]),
    "rg_encode_message": (_i, [C.POINTER(MessageC), C.c_char_p, _u64, C.POINTER(C.c_uint64)]),
    "rg_local_append": (_i, [_vp, _u64, _u64]),
    "rg_local_persisted": (_i, [_vp, _u64, _u64]),
    "rg_mark_sent": (_i, [_vp, _u64, _u64]),
    "rg_local_become_leader": (_i, [_vp, _u64, _u64]),
    "rg_flush": (_i, [_vp]),
    "rg_comm_unique_id": (_i, [_vp]),
    "rg_comm_init": (_i, [_vp, C.POINTER(CommConfig)]),
    "rg_comm_destroy": (_i, [_vp]),
    "rg_comm_warmup": (_i, []),
    "rg_comm_info_get": (_i, [_vp, C.POINTER(CommInfo)]),
    "rg_publish_commit": (_i, [_vp, C.c_uint32]),
    "rg_comm_init_all": (_i, [_vp, C.c_uint32, _vp]),
    "rg_publish_commit_all": (_i, [_vp, C.c_uint32, C.c_uint32]),
    "rg_publish_sync": (_i, [_vp]),
    "rg_published_commit_ptr": (_vp, [_vp, C.POINTER(_u64)]),
    "rg_published_commit": (_i, [_vp, C.c_uint32, _u64, _u64, _vp]),
    "rg_publish_stats_get": (_i, [_vp, C.POINTER(PublishStats)]),
    "rg_pub_bytes_per_rank": (_u64, [_u64, C.c_uint32]),
    "rg_pub_accumulate_host": (_i, [_u64, C.c_uint32, _vp, _vp, _vp]),
    "rg_pub_apply_host": (_i, [_u64, C.c_uint32, C.c_uint32, _vp, _vp, C.POINTER(C.c_uint32)]),
    "rg_workload_init": (_i, [_vp, C.POINTER(_Workload), _u64]),
    "rg_workload_gen": (_i, [_vp, C.POINTER(_Workload), _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
    "rg_workload_init_host": (_i, [C.POINTER(_Workload), _u64, C.POINTER(_HostState)]),
    "rg_workload_gen_host": (_i, [C.POINTER(_Workload), _u64, _u64, C.POINTER(_HostState), _vp, _vp, _vp, _vp, _vp]),
}

_lib = None


def load_library():
    """dlopen the in-tree HIP engine. Fails loudly when it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -m raft_rs_amd.build` "
                          "(hipcc, gfx950). The engine has no CPU fallback.")
    try:
        # torch ships its own HIP runtime; load it FIRST so the engine binds to the same runtime
        # instance (streams handed over with rg_set_stream must belong to it).
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if L.rg_abi_version() != ABI_VERSION:  # (the ABI is source-compatible only: struct layouts follow the header)
        raise ImportError(f"{LIB_PATH} was built with RG_ABI_VERSION {L.rg_abi_version()}, these bindings are written "
                          f"against {ABI_VERSION}: rebuild with `python -m raft_rs_amd.build --force`")
    # include/raftgroups_mirror.h: rgr_mirror_stats is an exported OBJECT that holds the function's address
    L.rgr_mirror_stats_fn = C.CFUNCTYPE(_i, _vp, C.POINTER(MirrorInfo))(C.c_void_p.in_dll(L, "rgr_mirror_stats").value)
    _lib = L
    return L


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data
    return int(a)


class MsgBuffers:
    """Host-side message columns of one tick (layout of rg_msgs)."""

    def __init__(self, n_groups, n_slots, stride):
        self.n_groups, self.n_slots, self.stride = n_groups, n_slots, stride
        self.m_index = np.zeros((n_slots, stride), dtype=np.uint64)
        self.m_commit = np.zeros((n_slots, stride), dtype=np.uint64)
        self.m_hint = np.zeros((n_slots, stride), dtype=np.uint64)
        self.m_rs = np.zeros((n_slots, stride), dtype=np.uint64)
        self.m_logterm = np.zeros((n_slots, stride), dtype=np.uint64)
        self.m_flags = np.zeros((n_groups, 8), dtype=np.uint8)

    def clear(self):
        for a in (self.m_index, self.m_commit, self.m_hint, self.m_rs, self.m_logterm, self.m_flags):
            a[...] = 0

    def as_dict(self):
        return {"n_groups": self.n_groups, "n_slots": self.n_slots, "stride": self.stride,
                "m_index": self.m_index, "m_commit": self.m_commit, "m_hint": self.m_hint,
                "m_rs": self.m_rs, "m_logterm": self.m_logterm, "m_flags": self.m_flags}


class Engine:
    """One shard of raft groups resident on one MI355X (rg_engine)."""

    # what Engine() passes for the rg_config fields a caller leaves out (config_defaults: the tests run whole suites of
    # engines under one cache policy / offset width this way -- through the config struct, not through the environment)
    _defaults = {"cache_policy": CACHE.AUTO, "flags": 0, "cache_resident_groups": 0}

    def __init__(self, n_groups, n_slots, device=0, variant=VARIANT_DEFAULT, max_inflight=0, cache_policy=None,
                 flags=None, cache_resident_groups=None):
        """max_inflight > 0: Inflights rings of that capacity live on the device (send_appends after each tick).
        cache_policy / cache_resident_groups / flags: rg_config's (CACHE.*, CFGF.*); device_info() reports the decision."""
        self.L = load_library()
        self.h = _vp()
        d = Engine._defaults
        from_default = cache_policy is None
        cache_policy = d["cache_policy"] if cache_policy is None else cache_policy
        flags = d["flags"] if flags is None else flags
        cache_resident_groups = d["cache_resident_groups"] if cache_resident_groups is None else cache_resident_groups
        if max_inflight and cache_policy == CACHE.RESIDENT and from_default:
            cache_policy = CACHE.STREAM_ALL  # (a suite-wide default the send-stage engines cannot take: rg_create refuses it)
        cfg = _Config(n_groups, n_slots, device, variant, max_inflight, cache_policy, flags, cache_resident_groups)
        self._check(self.L.rg_create(C.byref(cfg), C.byref(self.h)))
        self.n_groups, self.n_slots, self.device, self.max_inflight = n_groups, n_slots, device, max_inflight
        self.stride = self.L.rg_stride(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.L.rg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self.L.rg_last_error().decode())
        return rc

    # ---- plumbing --------------------------------------------------------------------------
    def set_stream(self, stream_handle):
        self._check(self.L.rg_set_stream(self.h, _vp(stream_handle)))

    def sync(self):
        self._check(self.L.rg_sync(self.h))

    def device_info(self):
        """hipGetDeviceProperties of the engine's device + the device memory the engine holds."""
        d = DeviceInfo()
        self._check(self.L.rg_get_device_info(self.h, C.byref(d)))
        return {"arch": d.arch.decode(), "compute_units": d.compute_units, "wavefront": d.wavefront,
                "lds_per_workgroup": d.lds_per_workgroup, "hbm_bytes": d.hbm_bytes, "l2_bytes": d.l2_bytes,
                "engine_bytes": d.engine_bytes, "cache_policy": CACHE.NAMES[d.cache_policy],
                "engines_on_device": d.engines_on_device, "resident_groups": d.resident_groups,
                "last_tick_kernel": KERNEL.NAMES[d.last_tick_kernel], "last_tick_streaming": d.last_tick_streaming,
                "infinity_cache_bytes": d.infinity_cache_bytes, "infinity_cache_queried": bool(d.infinity_cache_queried),
                "last_tick_offset_bits": d.last_tick_offset_bits}

    def column_shape_dtype(self, col):
        if col in COL.PER_SLOT:
            return (self.n_slots, self.stride), np.uint64
        if col in COL.PER_RUN:
            return (TERM_RUNS, self.stride), np.uint64
        if col == COL.PFLAGS:
            return (self.n_groups, 8), np.uint8
        if col in (COL.CFG, COL.OUT):
            return (self.n_groups,), np.uint32
        if col in (COL.HOST_HINT, COL.RUN_COUNT):
            return (self.n_groups,), np.uint8
        return (self.n_groups,), np.uint64

    def load_column(self, col, arr):
        shape, dt = self.column_shape_dtype(col)
        a = np.ascontiguousarray(arr, dtype=dt)
        assert a.shape == shape, (COL.NAMES[col], a.shape, shape)
        self._check(self.L.rg_load_column(self.h, col, a.ctypes.data, a.nbytes))

    def read_column(self, col):
        shape, dt = self.column_shape_dtype(col)
        a = np.empty(shape, dtype=dt)
        self._check(self.L.rg_read_column(self.h, col, a.ctypes.data, a.nbytes))
        return a

    def column_ptr(self, col):
        return self.L.rg_column_ptr(self.h, col)

    def load_state(self, st):
        """st: dict with the column names of COL.NAMES[:11] (numpy arrays shaped as column_shape_dtype says)."""
        for col in range(COL.CFG + 1):
            self.load_column(col, st[COL.NAMES[col]])
        for col in (COL.RUN_FIRST, COL.RUN_TERM, COL.DUMMY_INDEX, COL.DUMMY_TERM, COL.CUR_TERM):  # optional term-run table
            if COL.NAMES[col] in st:
                self.load_column(col, st[COL.NAMES[col]])

    def read_state(self):
        st = {"n_groups": self.n_groups, "n_slots": self.n_slots, "stride": self.stride}
        for col in range(COL.OUT + 1):
            st[COL.NAMES[col]] = self.read_column(col)
        return st

    def read_groups(self, groups):
        """Status of whole groups (all Progress cells, commit, log range, cfg, last result word) as a
        GROUP_STATUS_DTYPE array -- the sparse counterpart of read_state()."""
        ids = np.ascontiguousarray(groups, dtype=np.uint64)
        out = np.zeros(len(ids), dtype=GROUP_STATUS_DTYPE)
        self._check(self.L.rg_read_groups(self.h, ids.ctypes.data, len(ids), out.ctypes.data))
        return out

    def checkpoint(self):
        self._check(self.L.rg_checkpoint(self.h))

    def restore(self):
        self._check(self.L.rg_restore(self.h))

    def write_cells(self, cells):
        """cells: list of dicts {group, slot, <column name>: value, ...}."""
        arr = (CellWrite * max(1, len(cells)))()
        for i, c in enumerate(cells):
            arr[i].group, arr[i].slot = c["group"], c["slot"]
            mask = 0
            for col in range(COL.PFLAGS + 1):
                name = COL.NAMES[col]
                if name in c:
                    mask |= 1 << col
                    setattr(arr[i], name, int(c[name]))
            arr[i].field_mask = mask
        self._check(self.L.rg_write_cells(self.h, arr, len(cells)))

    def set_config(self, group, cfg_word):
        """apply_conf for one group: rewrite its RG_CFG_* word."""
        self._check(self.L.rg_set_config(self.h, group, int(cfg_word)))

    # ---- hot path --------------------------------------------------------------------------
    def tick(self, msgs):
        """Host-buffer tick (H2D copy + kernel + sync)."""
        m = _Msgs(_ptr(msgs.m_index), _ptr(msgs.m_commit), _ptr(msgs.m_hint), _ptr(msgs.m_rs), _ptr(msgs.m_flags),
                  _ptr(getattr(msgs, "m_logterm", None)))
        self._check(self.L.rg_tick(self.h, C.byref(m)))

    def tick_device(self, m_index, m_commit, m_hint, m_rs, m_flags, m_logterm=None):
        """Device-pointer tick (asynchronous on the engine's stream)."""
        m = _Msgs(_ptr(m_index), _ptr(m_commit), _ptr(m_hint), _ptr(m_rs), _ptr(m_flags), _ptr(m_logterm))
        self._check(self.L.rg_tick_device(self.h, C.byref(m)))

    def ingest(self, records):
        """records: numpy structured array of WIRE_DTYPE (wire-order AppendResponse records). Returns the
        number of dropped duplicate / malformed records."""
        rec = np.ascontiguousarray(records, dtype=WIRE_DTYPE)
        dup = _u64(0)
        self._check(self.L.rg_ingest(self.h, rec.ctypes.data, len(rec), C.byref(dup)))
        return dup.value

    def ingest_device(self, dev_records_ptr, n):
        self._check(self.L.rg_ingest_device(self.h, _ptr(dev_records_ptr), n))

    def ingested_duplicates(self):
        d = _u64(0)
        self._check(self.L.rg_ingested_duplicates(self.h, C.byref(d)))
        return d.value

    def tick_ingested(self):
        n = _u64(0)
        self._check(self.L.rg_tick_ingested(self.h, C.byref(n)))
        return n.value

    def ingest_tick(self, records):
        """ingest + tick_ingested in one host<->device round trip. Returns (groups touched, dropped records)."""
        rec = np.ascontiguousarray(records, dtype=WIRE_DTYPE)
        n, dup = _u64(0), _u64(0)
        self._check(self.L.rg_ingest_tick(self.h, rec.ctypes.data, len(rec), C.byref(n), C.byref(dup)))
        return n.value, dup.value

    def ingested_results(self, cap=None):
        """(groups, commit, out) of the last sparse tick. cap: hand rg_ingested_results arrays of that capacity instead of
        asking for the count first -> (groups, commit, out, n): arrays of length cap of which min(cap, n) are written
        (the rest keeps its 0xA5 fill), n the true count."""
        n = _u64(0)
        if cap is not None:
            groups = np.full(cap, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
            commit = np.full(cap, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
            out = np.full(cap, 0xA5A5A5A5, dtype=np.uint32)
            self._check(self.L.rg_ingested_results(self.h, groups.ctypes.data if cap else None,
                                                   commit.ctypes.data if cap else None, out.ctypes.data if cap else None,
                                                   cap, C.byref(n)))
            return groups, commit, out, n.value
        self._check(self.L.rg_ingested_results(self.h, None, None, None, 0, C.byref(n)))
        k = n.value
        groups = np.empty(k, dtype=np.uint64)
        commit = np.empty(k, dtype=np.uint64)
        out = np.empty(k, dtype=np.uint32)
        if k:
            self._check(self.L.rg_ingested_results(self.h, groups.ctypes.data, commit.ctypes.data, out.ctypes.data, k,
                                                   C.byref(n)))
        return groups, commit, out

    def tick_device_fused(self, ticks, dev_out_t, dev_commit_t=None):
        """ticks: list (1..8) of (m_index, m_commit, m_hint, m_rs, m_flags) DEVICE pointers in tick order;
        dev_out_t: device u32 [T][G]; dev_commit_t: optional device u64 [T][G]. Asynchronous. Returns the number of ticks
        applied: len(ticks), or fewer when a log-term tick raised RG_OUT_HOST_HINT and the call stopped behind it
        (RG_ERR_HOST_HINT; answer the hints, then submit the rest)."""
        arr = (_Msgs * len(ticks))()
        for i, t in enumerate(ticks):
            arr[i] = _Msgs(*([_ptr(x) for x in t] + [None] * (6 - len(t))))
        rc = self.L.rg_tick_device_fused(self.h, arr, len(ticks), _ptr(dev_out_t), _ptr(dev_commit_t))
        if rc != ERR["HOST_HINT"]:
            self._check(rc)
        return self.fused_ticks_done()

    def fused_ticks_done(self):
        n = C.c_uint32(0)
        self._check(self.L.rg_fused_ticks_done(self.h, C.byref(n)))
        return int(n.value)

    # ---- send stage (device Inflights + maybe_send_append decisions) ------------------------------
    def send_appends(self, max_entries_per_msg=0, skip_bcast_commit=False, max_bytes=None):
        """Run the send stage for the tick that just ran (asynchronous). max_bytes: Config::max_size_per_msg in bytes over
        the entry sizes on the device (RG_SEND_BYTES; NO_LIMIT = no limit) instead of the entries-per-message model."""
        flags = SEND_SKIP_BCAST_COMMIT if skip_bcast_commit else 0
        if max_bytes is not None:
            max_entries_per_msg, flags = max_bytes, flags | SEND_BYTES
        self._check(self.L.rg_send_appends(self.h, max_entries_per_msg, flags))

    def tick_send(self, msgs, max_entries_per_msg=0, skip_bcast_commit=False, max_bytes=None):
        """tick(msgs) + send_appends(...) as ONE launch (k_tick_send); host buffers, synchronises like tick()."""
        flags = SEND_SKIP_BCAST_COMMIT if skip_bcast_commit else 0
        if max_bytes is not None:
            max_entries_per_msg, flags = max_bytes, flags | SEND_BYTES
        m = _Msgs(_ptr(msgs.m_index), _ptr(msgs.m_commit), _ptr(msgs.m_hint), _ptr(msgs.m_rs), _ptr(msgs.m_flags),
                  _ptr(getattr(msgs, "m_logterm", None)))
        self._check(self.L.rg_tick_send(self.h, C.byref(m), max_entries_per_msg, flags))

    def tick_device_send(self, m_index, m_commit, m_hint, m_rs, m_flags, m_logterm=None, max_entries_per_msg=0,
                         skip_bcast_commit=False, max_bytes=None):
        """tick_device(...) + send_appends(...) as ONE launch; device pointers, asynchronous."""
        flags = SEND_SKIP_BCAST_COMMIT if skip_bcast_commit else 0
        if max_bytes is not None:
            max_entries_per_msg, flags = max_bytes, flags | SEND_BYTES
        m = _Msgs(_ptr(m_index), _ptr(m_commit), _ptr(m_hint), _ptr(m_rs), _ptr(m_flags), _ptr(m_logterm))
        self._check(self.L.rg_tick_device_send(self.h, C.byref(m), max_entries_per_msg, flags))

    def flush_send(self, max_entries_per_msg=0, skip_bcast_commit=False, max_bytes=None):
        """flush() + send_appends(); one host<->device round trip for small batches."""
        flags = SEND_SKIP_BCAST_COMMIT if skip_bcast_commit else 0
        if max_bytes is not None:
            max_entries_per_msg, flags = max_bytes, flags | SEND_BYTES
        self._check(self.L.rg_flush_send(self.h, max_entries_per_msg, flags))

    def mailbox_start(self, idle_timeout_us=0):
        """Keep one workgroup resident for small flushes (no launch / synchronisation per flush); see raftgroups.h."""
        self._check(self.L.rg_mailbox_start(self.h, idle_timeout_us))

    def mailbox_stop(self):
        self._check(self.L.rg_mailbox_stop(self.h))

    def mailbox_stats(self):
        """(flushes served by the resident workgroup, times it was launched)"""
        a, b = _u64(0), _u64(0)
        self._check(self.L.rg_mailbox_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def log_sizes_enable(self, window):
        """Byte-accurate max_size_per_msg: keep the cumulative sizes of every group's last `window` entries on the device."""
        self._check(self.L.rg_log_sizes_enable(self.h, window))

    def log_sizes_write(self, recs):
        """recs: LOG_SIZE_DTYPE array, one record per appended entry (cumulative bytes up to and including it)."""
        recs = np.ascontiguousarray(recs, dtype=LOG_SIZE_DTYPE)
        self._check(self.L.rg_log_sizes_write(self.h, recs.ctypes.data, len(recs)))

    def workload_sizes(self, seed, min_bytes, spread):
        self._check(self.L.rg_workload_sizes(self.h, seed, min_bytes, spread))

    def update_state(self, msgs):
        """msgs: SENT_MSG_DTYPE array of MsgAppends the HOST sent (RG_SEND_HOST items): Progress::update_state(last)."""
        msgs = np.ascontiguousarray(msgs, dtype=SENT_MSG_DTYPE)
        self._check(self.L.rg_update_state(self.h, msgs.ctypes.data, len(msgs)))

    def progress_events(self, events):
        """events: PROGRESS_EVENT_DTYPE array (or [(group, slot, kind)]): report_unreachable / report_snapshot in place."""
        events = np.ascontiguousarray(np.array(events, dtype=PROGRESS_EVENT_DTYPE))
        self._check(self.L.rg_progress_events(self.h, events.ctypes.data, len(events)))

    def progress_event_dense(self, kind, slot_plus1):
        """slot_plus1: u8 [G], 0 = nothing for the group, s + 1 = event `kind` goes to its slot s (rg_progress_event_dense)."""
        a = np.ascontiguousarray(slot_plus1, dtype=np.uint8)
        assert a.shape == (self.n_groups,)
        self._check(self.L.rg_progress_event_dense(self.h, kind, a.ctypes.data))

    def report_unreachable(self, group, peer_id):
        self._check(self.L.rg_report_unreachable(self.h, group, peer_id))

    def report_snapshot(self, group, peer_id, failure):
        self._check(self.L.rg_report_snapshot(self.h, group, peer_id, int(bool(failure))))

    def send_items(self):
        """Work items of the last send stage as a SEND_ITEM_DTYPE array (order unspecified)."""
        n = _u64(0)
        items = np.empty(4096, dtype=SEND_ITEM_DTYPE)  # small stages come back in one call
        self._check(self.L.rg_send_items(self.h, items.ctypes.data, len(items), C.byref(n)))
        if n.value > len(items):
            items = np.empty(n.value, dtype=SEND_ITEM_DTYPE)
            self._check(self.L.rg_send_items(self.h, items.ctypes.data, n.value, C.byref(n)))
        return items[:n.value]

    def send_columns(self):
        """Device pointers (prev_index u64 [P][stride], last_index u64 [P][stride], n_msgs | kind << 16 u32 [P][stride])
        of the last DENSE stage's work items."""
        a, b, c = _vp(), _vp(), _vp()
        self._check(self.L.rg_send_columns(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def send_tail_column(self):
        """Device pointer of the windows' newest-inflight column (u64 [P][stride]): where an item whose n / kind word has bit 31
        (SEND_LAST_IS_TAIL) keeps its last_index."""
        a = _vp()
        self._check(self.L.rg_send_tail_column(self.h, C.byref(a)))
        return a.value

    def read_inflights(self):
        """(meta u32 [P][stride] = start | count << 16, ring u64 [G][P][cap])."""
        meta = np.empty((self.n_slots, self.stride), dtype=np.uint32)
        ring = np.empty((self.n_groups, self.n_slots, self.max_inflight), dtype=np.uint64)
        self._check(self.L.rg_read_inflights(self.h, meta.ctypes.data, ring.ctypes.data))
        return meta, ring

    def load_inflights(self, meta, ring):
        meta = np.ascontiguousarray(meta, dtype=np.uint32)
        ring = np.ascontiguousarray(ring, dtype=np.uint64)
        assert meta.shape == (self.n_slots, self.stride) and ring.shape == (self.n_groups, self.n_slots, self.max_inflight)
        self._check(self.L.rg_load_inflights(self.h, meta.ctypes.data, ring.ctypes.data))

    def inflights(self, group, slot, meta=None, ring=None):
        """Logical contents (oldest first) of one Progress's Inflights."""
        if meta is None:
            meta, ring = self.read_inflights()
        m = int(meta[slot, group])
        start, count = m & 0xffff, m >> 16
        return [int(ring[group, slot, (start + i) % self.max_inflight]) for i in range(count)]

    def recompute(self):
        self._check(self.L.rg_recompute(self.h))

    def maximal_committed_index(self, with_flag=False):
        mci = np.empty(self.n_groups, dtype=np.uint64)
        gc = np.empty(self.n_groups, dtype=np.uint8) if with_flag else None
        self._check(self.L.rg_maximal_committed_index(self.h, mci.ctypes.data, _ptr(gc)))
        return (mci, gc) if with_flag else mci

    def heartbeat_commits(self, dev_out=None):
        """bcast_heartbeat: min(matched, committed) per slot -> [P][stride] u64 (host copy). dev_out: a DEVICE pointer to
        u64 [P][stride] that receives the column instead (asynchronous on the engine's stream; returns None)."""
        if dev_out is not None:
            self._check(self.L.rg_heartbeat_commits(self.h, _ptr(dev_out), None))
            return None
        hb = np.empty((self.n_slots, self.stride), dtype=np.uint64)
        self._check(self.L.rg_heartbeat_commits(self.h, None, hb.ctypes.data))
        return hb

    def step_heartbeat_response(self, group, from_, term, commit=0, ins_full=False):
        self._check(self.L.rg_step_heartbeat_response(self.h, group, from_, term, commit, int(ins_full)))

    def results(self):
        commit = np.empty(self.n_groups, dtype=np.uint64)
        out = np.empty(self.n_groups, dtype=np.uint32)
        self._check(self.L.rg_results(self.h, commit.ctypes.data, out.ctypes.data))
        return commit, out

    def result_counts(self):
        a, b = _u64(0), _u64(0)
        self._check(self.L.rg_result_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def size_classes(self):
        """rg_size_classes: the ranges of the shard the next dense tick treats as one size class each -> [(first_group, n_groups,
        n_slots)]; [] = the plain kernel runs."""
        dt = np.dtype([("first_group", "<u8"), ("n_groups", "<u8"), ("n_slots", "<u4"), ("reserved", "<u4")])
        out = np.zeros(64, dtype=dt)
        n = C.c_uint32(0)
        self._check(self.L.rg_size_classes(self.h, out.ctypes.data, len(out), C.byref(n)))
        if n.value > len(out):
            out = np.zeros(n.value, dtype=dt)
            self._check(self.L.rg_size_classes(self.h, out.ctypes.data, len(out), C.byref(n)))
        return [(int(r["first_group"]), int(r["n_groups"]), int(r["n_slots"])) for r in out[:n.value]]

    def permute_groups(self, perm):
        """rg_permute_groups: group i becomes the group that was at perm[i] -- every column, the Inflights, the mirror's tables."""
        perm = np.ascontiguousarray(perm, dtype=np.uint64)
        assert perm.shape == (self.n_groups,)
        self._check(self.L.rg_permute_groups(self.h, perm.ctypes.data))

    def place_by_size_class(self):
        """Plan from the engine's own cfg column (rg_plan_placement) and permute: a shard loaded with its replica-set sizes
        interleaved becomes the layout the one-launch class kernel runs. Returns (perm, the planned ranges)."""
        perm, classes = plan_placement(self.read_column(COL.CFG), self.n_slots)
        self.permute_groups(perm)
        return perm, classes

    def host_hints(self, cap=None):
        """Groups whose last tick raised RG_OUT_HOST_HINT -> HOST_HINT_DTYPE array (group, slot_mask). cap: hand rg_host_hints an
        array of that capacity (cap = 0: no array at all) instead of asking again -> (items, n): an array of length cap of which
        min(cap, n) entries are written (the rest keeps its 0xA5 fill), n the true count."""
        n = _u64(0)
        if cap is not None:
            items = np.frombuffer(bytes([0xA5]) * (cap * HOST_HINT_DTYPE.itemsize), dtype=HOST_HINT_DTYPE).copy()
            self._check(self.L.rg_host_hints(self.h, items.ctypes.data if cap else None, cap, C.byref(n)))
            return items, n.value
        items = np.zeros(256, dtype=HOST_HINT_DTYPE)
        self._check(self.L.rg_host_hints(self.h, items.ctypes.data, len(items), C.byref(n)))
        if n.value > len(items):
            items = np.zeros(n.value, dtype=HOST_HINT_DTYPE)
            self._check(self.L.rg_host_hints(self.h, items.ctypes.data, len(items), C.byref(n)))
        return items[:n.value]

    def resolve_host_hints(self, recs):
        """recs: RESOLVED_HINT_DTYPE array (or [(group, index, hint, slot, 0)]): the host's find_conflict_by_term answers.
        Returns u8[n]: maybe_decr_to returned true (send_append is due)."""
        recs = np.ascontiguousarray(np.array(recs, dtype=RESOLVED_HINT_DTYPE))
        applied = np.zeros(len(recs), dtype=np.uint8)
        self._check(self.L.rg_resolve_host_hints(self.h, recs.ctypes.data, len(recs), applied.ctypes.data))
        return applied

    def msg_stats(self, dev_m_flags):
        c = (_u64 * 5)()
        self._check(self.L.rg_msg_stats(self.h, _ptr(dev_m_flags), C.byref(c)))
        return {"valid": c[0], "rejects": c[1], "slots": c[2], "groups_with_events": c[3], "elections": c[4]}

    def vote_result(self, yes, no):
        yes = np.ascontiguousarray(yes, dtype=np.uint8)
        no = np.ascontiguousarray(no, dtype=np.uint8)
        res = np.empty(self.n_groups, dtype=np.uint8)
        self._check(self.L.rg_vote_result(self.h, yes.ctypes.data, no.ctypes.data, res.ctypes.data))
        return res

    def tally_votes(self, yes, no):
        """ProgressTracker::tally_votes: (granted, rejected, result) per group."""
        yes = np.ascontiguousarray(yes, dtype=np.uint8)
        no = np.ascontiguousarray(no, dtype=np.uint8)
        g, r, res = (np.empty(self.n_groups, dtype=np.uint8) for _ in range(3))
        self._check(self.L.rg_tally_votes(self.h, yes.ctypes.data, no.ctypes.data, g.ctypes.data, r.ctypes.data,
                                          res.ctypes.data))
        return g, r, res

    def quorum_recently_active(self):
        res = np.empty(self.n_groups, dtype=np.uint8)
        self._check(self.L.rg_quorum_recently_active(self.h, res.ctypes.data))
        return res

    # ---- ReadIndex: pending-read queues and the ack quorum on the device ---------------------------
    def read_index_enable(self, depth):
        """rg_read_index_enable: one FIFO of `depth` (1..16) pending reads per group."""
        self._check(self.L.rg_read_index_enable(self.h, depth))

    def read_index(self, reqs, lease=False):
        """Step MsgReadIndex requests: reqs is a READ_REQ_DTYPE array (or [(group, ctx)]) -> u8[n] of READ_* statuses."""
        reqs = np.ascontiguousarray(np.array(reqs, dtype=READ_REQ_DTYPE))
        status = np.zeros(len(reqs), dtype=np.uint8)
        self._check(self.L.rg_read_index(self.h, reqs.ctypes.data, len(reqs), READ_LEASE if lease else 0, status.ctypes.data))
        return status

    def read_acks(self, acks):
        """The read-only halves of heartbeat responses: a READ_ACK_DTYPE array (or [(group, ctx, slot, flags)])."""
        acks = np.ascontiguousarray(np.array(acks, dtype=READ_ACK_DTYPE))
        self._check(self.L.rg_read_acks(self.h, acks.ctypes.data, len(acks)))

    def read_acks_device(self, dev_ctx):
        """One heartbeat round of every group: dev_ctx = device pointer to u64 [P][stride] context handles (asynchronous)."""
        self._check(self.L.rg_read_acks_device(self.h, _ptr(dev_ctx)))

    def read_states(self, cap=None):
        """Drain the list of read states -> READ_STATE_DTYPE array. With `cap`: (the first cap states, how many there were)."""
        n = _u64(0)
        if cap is not None:
            items = np.zeros(cap, dtype=READ_STATE_DTYPE)
            self._check(self.L.rg_read_states(self.h, items.ctypes.data, cap, C.byref(n)))
            return items[:min(cap, n.value)], n.value
        self._check(self.L.rg_read_states(self.h, None, 0, C.byref(n)))  # (cap = 0 only counts)
        items = np.zeros(max(n.value, 1), dtype=READ_STATE_DTYPE)
        self._check(self.L.rg_read_states(self.h, items.ctypes.data, len(items), C.byref(n)))
        return items[:n.value]

    def read_last_pending(self):
        """last_pending_request_ctx per group (0 = none): what a regular bcast_heartbeat attaches -> u64[G] (host copy)."""
        ctx = np.empty(self.n_groups, dtype=np.uint64)
        self._check(self.L.rg_read_last_pending(self.h, None, ctx.ctypes.data))
        return ctx

    def read_pending_counts(self):
        """pending_read_count per group -> u8[G]."""
        counts = np.empty(self.n_groups, dtype=np.uint8)
        self._check(self.L.rg_read_pending_counts(self.h, counts.ctypes.data))
        return counts

    # ---- the follower half: MsgAppend / MsgHeartbeat steps of the groups this store follows ---------
    def follow_enable(self, n_follow):
        """rg_follow_enable: the arena of n_follow followed groups (an index space of its own). Once."""
        self._check(self.L.rg_follow_enable(self.h, n_follow))

    def follow_stride(self):
        return self.L.rg_follow_stride(self.h)

    def follow_write(self, states):
        """Load whole group states: a FOLLOW_STATE_DTYPE array (canonical, or EngineError)."""
        states = np.ascontiguousarray(states, dtype=FOLLOW_STATE_DTYPE)
        self._check(self.L.rg_follow_write(self.h, states.ctypes.data, len(states)))

    def follow_read(self, groups):
        """Whole group states of `groups` -> FOLLOW_STATE_DTYPE array."""
        groups = np.ascontiguousarray(groups, dtype=np.uint64)
        out = np.zeros(len(groups), dtype=FOLLOW_STATE_DTYPE)
        self._check(self.L.rg_follow_read(self.h, groups.ctypes.data, len(groups), out.ctypes.data))
        return out

    def follow_step(self, msgs, ext=None):
        """Sparse step: msgs is a FOLLOW_MSG_DTYPE array (any groups, array order per group), ext a FOLLOW_ENT_RUN_DTYPE array
        of the further entry runs -> FOLLOW_RESP_DTYPE array, positional."""
        msgs = np.ascontiguousarray(msgs, dtype=FOLLOW_MSG_DTYPE)
        n_ext = 0 if ext is None else len(ext)
        if n_ext:
            ext = np.ascontiguousarray(ext, dtype=FOLLOW_ENT_RUN_DTYPE)
        resp = np.zeros(len(msgs), dtype=FOLLOW_RESP_DTYPE)
        self._check(self.L.rg_follow_step(self.h, msgs.ctypes.data, len(msgs), ext.ctypes.data if n_ext else None, n_ext, resp.ctypes.data))
        return resp

    def _follow_msgs(self, msgs):
        return FollowMsgs(*[self._dev_ptr(msgs.get(k)) for k in ("flags", "index", "log_term", "commit", "ent_term", "n_entries", "ext", "ext_runs")],
                          int(msgs.get("n_ext", 0)))

    def _follow_out(self, out):
        return FollowOut(*[self._dev_ptr(out.get(k)) for k in ("status", "index", "commit", "conflict", "reject_hint", "log_term")])

    def follow_step_device(self, msgs, out):
        """Dense step (asynchronous): msgs / out are dicts of DEVICE pointers (ints or objects with data_ptr()) named as the
        fields of rg_follow_msgs / rg_follow_out; msgs may leave out ext / ext_runs / n_ext."""
        m, o = self._follow_msgs(msgs), self._follow_out(out)
        self._check(self.L.rg_follow_step_device(self.h, C.byref(m), C.byref(o)))

    # ---- the follower's term gate, vote step and election clock ------------------------------------
    def follow_gate_enable(self, election_tick, min_timeout=0, max_timeout=0, flags=0, seed=0):
        """rg_follow_gate_enable: the soft cells of every followed group. Once, after follow_enable."""
        cfg = FollowGateConfig(election_tick, min_timeout, max_timeout, flags, seed)
        self._check(self.L.rg_follow_gate_enable(self.h, C.byref(cfg)))

    def follow_soft_write(self, soft):
        """Load soft states: a FOLLOW_SOFT_DTYPE array (distinct groups; randomized_timeout 0 = draw one)."""
        soft = np.ascontiguousarray(soft, dtype=FOLLOW_SOFT_DTYPE)
        self._check(self.L.rg_follow_soft_write(self.h, soft.ctypes.data, len(soft)))

    def follow_soft_read(self, groups):
        groups = np.ascontiguousarray(groups, dtype=np.uint64)
        out = np.zeros(len(groups), dtype=FOLLOW_SOFT_DTYPE)
        self._check(self.L.rg_follow_soft_read(self.h, groups.ctypes.data, len(groups), out.ctypes.data))
        return out

    def follow_step_gated(self, msgs, hdrs, ext=None):
        """Sparse gated step, all five kinds: msgs (FOLLOW_MSG_DTYPE) and hdrs (FOLLOW_HDR_DTYPE), positional ->
        (FOLLOW_RESP_DTYPE array, FOLLOW_GATE_RESP_DTYPE array)."""
        msgs = np.ascontiguousarray(msgs, dtype=FOLLOW_MSG_DTYPE)
        hdrs = np.ascontiguousarray(hdrs, dtype=FOLLOW_HDR_DTYPE)
        if len(hdrs) != len(msgs):
            raise ValueError("one header per record")
        n_ext = 0 if ext is None else len(ext)
        if n_ext:
            ext = np.ascontiguousarray(ext, dtype=FOLLOW_ENT_RUN_DTYPE)
        resp = np.zeros(len(msgs), dtype=FOLLOW_RESP_DTYPE)
        gate = np.zeros(len(msgs), dtype=FOLLOW_GATE_RESP_DTYPE)
        self._check(self.L.rg_follow_step_gated(self.h, msgs.ctypes.data, hdrs.ctypes.data, len(msgs), ext.ctypes.data if n_ext else None, n_ext,
                                                resp.ctypes.data, gate.ctypes.data))
        return resp, gate

    def follow_step_gated_device(self, msgs, term, from_, out, gate, events, resp_term):
        """Dense gated step (asynchronous): as follow_step_device, with the DEVICE columns term / from_ (u64) and the outputs
        gate / events (u8) and resp_term (u64)."""
        p = self._dev_ptr
        m, o = self._follow_msgs(msgs), self._follow_out(out)
        self._check(self.L.rg_follow_step_gated_device(self.h, C.byref(m), p(term), p(from_), C.byref(o), p(gate), p(events), p(resp_term)))

    def follow_clock(self, hup, cap, sync=True):
        """rg_follow_clock: one Raft::tick of every followed group; hup = DEVICE u64 [cap] (None with cap 0). sync: -> the number
        appended; else asynchronous, the counts are the two device words at follow_clock_counts()."""
        n = C.c_uint64(0)
        self._check(self.L.rg_follow_clock(self.h, self._dev_ptr(hup), cap, C.byref(n) if sync else None))
        return n.value if sync else None

    def follow_clock_counts(self):
        """Device address of u64 [2]: groups appended, groups due, of the last follow_clock."""
        return self.L.rg_follow_clock_counts(self.h)

    # ---- the candidate half: campaign, vote responses and poll -------------------------------------
    def follow_elect_enable(self):
        """rg_follow_elect_enable: the election cells of every followed group. Once, after follow_gate_enable."""
        self._check(self.L.rg_follow_elect_enable(self.h))

    def follow_elect_write(self, cells):
        """Load election cells: a FOLLOW_ELECT_DTYPE array (distinct groups, self_id != 0, no slot both yes and no)."""
        cells = np.ascontiguousarray(cells, dtype=FOLLOW_ELECT_DTYPE)
        self._check(self.L.rg_follow_elect_write(self.h, cells.ctypes.data, len(cells)))

    def follow_elect_read(self, groups):
        groups = np.ascontiguousarray(groups, dtype=np.uint64)
        out = np.zeros(len(groups), dtype=FOLLOW_ELECT_DTYPE)
        self._check(self.L.rg_follow_elect_read(self.h, groups.ctypes.data, len(groups), out.ctypes.data))
        return out

    @staticmethod
    def _dev_ptr(x):
        return None if x is None else int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x)

    def follow_campaign_device(self, groups, n, cap, out, block=None):
        """rg_follow_campaign_device (asynchronous): MsgHup for min(*n, cap) groups of the DEVICE list `groups`; n = a device u64
        (follow_clock_counts()), block = a DEVICE u8 [stride] column or None, out = a dict of DEVICE columns named as
        ELECT_OUT_COLUMNS, indexed by list position."""
        p = self._dev_ptr
        o = FollowElectOut(*[p(out.get(k)) for k in ELECT_OUT_COLUMNS])
        self._check(self.L.rg_follow_campaign_device(self.h, p(groups), p(n), cap, p(block), C.byref(o)))

    def follow_campaign(self, reqs):
        """Sparse MsgHup / MsgTimeoutNow records: a FOLLOW_CAMPAIGN_REQ_DTYPE array (distinct groups) -> FOLLOW_ELECT_RESP_DTYPE
        array, positional."""
        reqs = np.ascontiguousarray(reqs, dtype=FOLLOW_CAMPAIGN_REQ_DTYPE)
        resp = np.zeros(len(reqs), dtype=FOLLOW_ELECT_RESP_DTYPE)
        self._check(self.L.rg_follow_campaign(self.h, reqs.ctypes.data, len(reqs), resp.ctypes.data))
        return resp

    def follow_vote_resps(self, recs):
        """Sparse vote responses: a FOLLOW_VOTE_REC_DTYPE array (any groups, array order per group) -> FOLLOW_ELECT_RESP_DTYPE
        array, positional."""
        recs = np.ascontiguousarray(recs, dtype=FOLLOW_VOTE_REC_DTYPE)
        resp = np.zeros(len(recs), dtype=FOLLOW_ELECT_RESP_DTYPE)
        self._check(self.L.rg_follow_vote_resps(self.h, recs.ctypes.data, len(recs), resp.ctypes.data))
        return resp

    def follow_vote_resps_device(self, msgs, out):
        """Dense vote responses (asynchronous): msgs / out are dicts of DEVICE columns named as VOTE_COLUMNS / ELECT_OUT_COLUMNS,
        [follow_stride()] each, indexed by group."""
        p = self._dev_ptr
        m = FollowVoteCols(*[p(msgs.get(k)) for k in VOTE_COLUMNS])
        o = FollowElectOut(*[p(out.get(k)) for k in ELECT_OUT_COLUMNS])
        self._check(self.L.rg_follow_vote_resps_device(self.h, C.byref(m), C.byref(o)))

    # ---- the hand-off between the follower arena and the leader columns ----------------------------
    def follow_promote(self, recs):
        """Sparse promotion of followed groups that won their election: a HANDOFF_REC_DTYPE array (distinct follow groups,
        distinct lead groups) -> HANDOFF_RESP_DTYPE array, positional. Synchronises."""
        recs = np.ascontiguousarray(recs, dtype=HANDOFF_REC_DTYPE)
        resp = np.zeros(len(recs), dtype=HANDOFF_RESP_DTYPE)
        self._check(self.L.rg_follow_promote(self.h, recs.ctypes.data, len(recs), resp.ctypes.data))
        return resp

    def follow_promote_device(self, result, lead, out, persisted=None):
        """Dense promotion (asynchronous): result = the DEVICE u8 `result` column follow_vote_resps_device wrote, lead = a DEVICE
        u64 column of lead groups, persisted = a DEVICE u64 column or None (the host vouches for persisted == last_index), out = a
        dict of DEVICE columns named as HANDOFF_OUT_COLUMNS; [follow_stride()] each, indexed by follow group."""
        p = self._dev_ptr
        o = HandoffOut(*[p(out.get(k)) for k in HANDOFF_OUT_COLUMNS])
        self._check(self.L.rg_follow_promote_device(self.h, p(result), p(lead), p(persisted), C.byref(o)))

    def follow_promote_send(self, recs, max_entries_per_msg=0, flags=0, item_cap=None):
        """rgh_follow_promote: the sparse promotion of an engine with device Inflights -- the promotion, the window resets and the
        first appends in one launch. -> (HANDOFF_RESP_DTYPE array, the first min(total, item_cap) work items as a SEND_ITEM_DTYPE
        array, the total number of items). item_cap None = room for every item. Synchronises."""
        recs = np.ascontiguousarray(recs, dtype=HANDOFF_REC_DTYPE)
        resp = np.zeros(len(recs), dtype=HANDOFF_RESP_DTYPE)
        cap = len(recs) * self.n_slots if item_cap is None else int(item_cap)
        items = np.zeros(cap, dtype=SEND_ITEM_DTYPE)
        n = C.c_uint64(0)
        self._check(self.L.rgh_follow_promote(self.h, recs.ctypes.data, len(recs), resp.ctypes.data, int(max_entries_per_msg), int(flags),
                                              items.ctypes.data if cap else None, cap, C.byref(n)))
        return resp, items[:min(n.value, cap)], n.value

    def follow_promote_send_device(self, result, lead, out, items, item_cap, count, persisted=None, max_entries_per_msg=0, flags=0):
        """rgh_follow_promote_device (asynchronous): result / lead / persisted / out as in follow_promote_device; items = a DEVICE
        buffer of item_cap SEND_ITEM_DTYPE records (None with item_cap 0), count = a DEVICE u32 the call zeroes and then holds the
        total number of items."""
        p = self._dev_ptr
        o = PromoteOut(HandoffOut(*[p(out.get(k)) for k in HANDOFF_OUT_COLUMNS]), p(items), int(item_cap), p(count))
        self._check(self.L.rgh_follow_promote_device(self.h, p(result), p(lead), p(persisted), int(max_entries_per_msg), int(flags), C.byref(o)))

    def apply_conf(self, recs, max_entries_per_msg=0, flags=0, item_cap=None):
        """rgc_apply_conf: apply_conf and post_conf_change for the led groups of `recs` (CONF_REC_DTYPE: group, cfg =
        cfg_make(incoming, outgoing, present=...) with every other field 0) in one launch. -> (CONF_RESP_DTYPE array, positional, the
        first min(total, item_cap) work items as a SEND_ITEM_DTYPE array, the total number of items). On an engine without device
        Inflights there are no items (item_cap must stay None or 0). Synchronises."""
        recs = np.ascontiguousarray(recs, dtype=CONF_REC_DTYPE)
        resp = np.zeros(len(recs), dtype=CONF_RESP_DTYPE)
        if not self.max_inflight:
            if item_cap:
                raise ValueError("apply_conf: an engine without device Inflights produces no work items")
            self._check(self.L.rgc_apply_conf(self.h, recs.ctypes.data, len(recs), resp.ctypes.data, int(max_entries_per_msg), int(flags), None, 0, None))
            return resp, np.zeros(0, dtype=SEND_ITEM_DTYPE), 0
        cap = len(recs) * self.n_slots if item_cap is None else int(item_cap)
        items = np.zeros(cap, dtype=SEND_ITEM_DTYPE)
        n = C.c_uint64(0)
        self._check(self.L.rgc_apply_conf(self.h, recs.ctypes.data, len(recs), resp.ctypes.data, int(max_entries_per_msg), int(flags),
                                          items.ctypes.data if cap else None, cap, C.byref(n)))
        return resp, items[:min(n.value, cap)], n.value

    def apply_conf_device(self, sel, cfg, status, events=None, commit=None, items=None, item_cap=0, count=None, max_entries_per_msg=0, flags=0):
        """rgc_apply_conf_device (asynchronous): sel = a DEVICE u8 column [n_groups] (0 = not selected), cfg = a DEVICE u32 column of
        the new words, status (mandatory) / events / commit = DEVICE columns [n_groups]; items = a DEVICE buffer of item_cap
        SEND_ITEM_DTYPE records (None with item_cap 0), count = a DEVICE u32 the call zeroes and then holds the total number of items
        (both None on an engine without device Inflights)."""
        p = self._dev_ptr
        o = ConfOut(p(status), p(events), p(commit), p(items), int(item_cap), p(count))
        self._check(self.L.rgc_apply_conf_device(self.h, p(sel), p(cfg), int(max_entries_per_msg), int(flags), C.byref(o)))

    def mirror_stats(self):
        """rgr_mirror_stats: the dense tick's read mirror -- launches that read the packed plane, launches that (re)built it, its
        size, whether it exists / is valid / is off for good. Host-side counters: no device work, the mirror stays as it is."""
        m = MirrorInfo()
        self._check(self.L.rgr_mirror_stats_fn(self.h, C.byref(m)))
        return {k: int(getattr(m, k)) for k, _ in MirrorInfo._fields_ if k != "version"}

    def transfer_leader(self, recs, max_entries=0, flags=0, item_cap=None):
        """rgm_transfer_leader: handle_transfer_leader for the led groups of `recs` (TRANSFER_REC_DTYPE: group, slot = the transferee)
        in one launch. -> (TRANSFER_RESP_DTYPE array, positional, the first min(total, item_cap) work items as a SEND_ITEM_DTYPE
        array, the total number of items). On an engine without device Inflights there are no items (item_cap must stay None or 0).
        Synchronises."""
        recs = np.ascontiguousarray(recs, dtype=TRANSFER_REC_DTYPE)
        resp = np.zeros(len(recs), dtype=TRANSFER_RESP_DTYPE)
        if not self.max_inflight:
            if item_cap:
                raise ValueError("transfer_leader: an engine without device Inflights produces no work items")
            self._check(self.L.rgm_transfer_leader(self.h, recs.ctypes.data, len(recs), resp.ctypes.data, int(max_entries), int(flags), None, 0, None))
            return resp, np.zeros(0, dtype=SEND_ITEM_DTYPE), 0
        cap = len(recs) if item_cap is None else int(item_cap)
        items = np.zeros(cap, dtype=SEND_ITEM_DTYPE)
        n = C.c_uint64(0)
        self._check(self.L.rgm_transfer_leader(self.h, recs.ctypes.data, len(recs), resp.ctypes.data, int(max_entries), int(flags),
                                               items.ctypes.data if cap else None, cap, C.byref(n)))
        return resp, items[:min(n.value, cap)], n.value

    def transfer_leader_device(self, to, status, events=None, items=None, item_cap=0, count=None, max_entries=0, flags=0):
        """rgm_transfer_leader_device (asynchronous): to = a DEVICE u8 column [n_groups] (0 = not selected, else the transferee's
        slot + 1), status (mandatory) / events = DEVICE u8 columns [n_groups]; items = a DEVICE buffer of item_cap SEND_ITEM_DTYPE
        records (None with item_cap 0), count = a DEVICE u32 the call zeroes and then holds the total number of items (both None on
        an engine without device Inflights)."""
        p = self._dev_ptr
        o = TransferOut(p(status), p(events), p(items), int(item_cap), p(count))
        self._check(self.L.rgm_transfer_leader_device(self.h, p(to), int(max_entries), int(flags), C.byref(o)))

    def follow_demote(self, recs):
        """Sparse demotion: the arena's log summary of follow_group is refreshed from lead_group (persisted unused) ->
        HANDOFF_RESP_DTYPE array, positional. Synchronises."""
        recs = np.ascontiguousarray(recs, dtype=HANDOFF_REC_DTYPE)
        resp = np.zeros(len(recs), dtype=HANDOFF_RESP_DTYPE)
        self._check(self.L.rg_follow_demote(self.h, recs.ctypes.data, len(recs), resp.ctypes.data))
        return resp

    def follow_demote_device(self, select, lead, out):
        """Dense demotion (asynchronous): the groups where the DEVICE u8 column `select` is non-zero; lead / out as in
        follow_promote_device."""
        p = self._dev_ptr
        o = HandoffOut(*[p(out.get(k)) for k in HANDOFF_OUT_COLUMNS])
        self._check(self.L.rg_follow_demote_device(self.h, p(select), p(lead), C.byref(o)))

    # ---- the leader's clock and the step-down ------------------------------------------------------
    def lead_clock_enable(self, election_tick, heartbeat_tick, flags=0):
        """rgx_lead_clock_enable: the clock cells of every group of the leader engine. Once. flags: GATE_CHECK_QUORUM |
        LEAD_CLOCK_START_LED."""
        cfg = LeadClockConfig(election_tick, heartbeat_tick, flags, 0)
        self._check(self.L.rgx_lead_clock_enable(self.h, C.byref(cfg)))

    def lead_clock_write(self, cells):
        """Load clock cells: a LEAD_CLOCK_CELL_DTYPE array (distinct groups, both counters below their timeouts)."""
        cells = np.ascontiguousarray(cells, dtype=LEAD_CLOCK_CELL_DTYPE)
        self._check(self.L.rgx_lead_clock_write(self.h, cells.ctypes.data, len(cells)))

    def lead_clock_read(self, groups):
        groups = np.ascontiguousarray(groups, dtype=np.uint64)
        out = np.zeros(len(groups), dtype=LEAD_CLOCK_CELL_DTYPE)
        self._check(self.L.rgx_lead_clock_read(self.h, groups.ctypes.data, len(groups), out.ctypes.data))
        return out

    def lead_clock(self, events, beat=None, beat_cap=0, down=None, down_cap=0, hb_commit=None, sync=True):
        """rgx_lead_clock: one Raft::tick of every led group. events = DEVICE u8 [n_groups]; beat / down = DEVICE u64 lists of
        beat_cap / down_cap places or None; hb_commit = DEVICE u64 [P][stride] or None. sync: -> (beats, check-quorum runs,
        step-downs, transfers aborted); else asynchronous, the counts are the four device words at lead_clock_counts()."""
        p = self._dev_ptr
        o = LeadClockOut(p(events), p(beat), beat_cap, p(down), down_cap, p(hb_commit))
        counts = (C.c_uint64 * 4)()
        self._check(self.L.rgx_lead_clock(self.h, C.byref(o), counts if sync else None))
        return tuple(int(x) for x in counts) if sync else None

    def lead_clock_counts(self):
        """Device address of u64 [4]: beats, check-quorum runs, step-downs, transfers aborted of the last lead_clock."""
        return self.L.rgx_lead_clock_counts(self.h)

    def follow_step_down(self, recs):
        """Sparse step-down: demotion of lead_group into follow_group plus become_follower(term, 0) on its soft cells (persisted
        unused) -> HANDOFF_RESP_DTYPE array, positional. Synchronises."""
        recs = np.ascontiguousarray(recs, dtype=HANDOFF_REC_DTYPE)
        resp = np.zeros(len(recs), dtype=HANDOFF_RESP_DTYPE)
        self._check(self.L.rgx_follow_step_down(self.h, recs.ctypes.data, len(recs), resp.ctypes.data))
        return resp

    def follow_step_down_device(self, events, lead, out):
        """Dense step-down (asynchronous): events = the DEVICE u8 [n_groups] column lead_clock wrote, lead = a DEVICE u64
        [follow_stride()] column of lead groups by follow group (HANDOFF_NO_LEAD = none), out as in follow_promote_device."""
        p = self._dev_ptr
        o = HandoffOut(*[p(out.get(k)) for k in HANDOFF_OUT_COLUMNS])
        self._check(self.L.rgx_follow_step_down_device(self.h, p(events), p(lead), C.byref(o)))

    # ---- the leader's term gate and the deposition --------------------------------------------------
    def lead_gate_device(self, m_flags, m_term, events, new_term, flags=None, down=None, down_cap=0, sync=True):
        """rgt_lead_gate_device: the term check of Raft::step for every record of a dense leader tick, in front of tick_device.
        m_flags = DEVICE u8 [n_groups][8] (the tick's RG_MF_* rows), m_term = DEVICE u64 [P][stride] (Message.term per record);
        events = DEVICE u8 [n_groups], new_term = DEVICE u64 [n_groups] (written where DEPOSED), flags = the DEVICE column the
        filtered rows go to (None: in place, over m_flags), down = DEVICE u64 list of down_cap places or None. sync: -> (groups
        deposed, stale records dropped, records of not-led groups dropped); else asynchronous, the counts are the three device
        words at lead_gate_counts()."""
        p = self._dev_ptr
        m = _Msgs(None, None, None, None, p(m_flags), None)
        o = TermGateOut(p(m_flags if flags is None else flags), p(events), p(new_term), p(down), down_cap)
        counts = (C.c_uint64 * 3)()
        self._check(self.L.rgt_lead_gate_device(self.h, C.byref(m), p(m_term), C.byref(o), counts if sync else None))
        return tuple(int(x) for x in counts) if sync else None

    def lead_gate_counts(self):
        """Device address of u64 [3]: groups deposed, stale records dropped, records of not-led groups dropped by the last gate."""
        return self.L.rgt_lead_gate_counts(self.h)

    def follow_depose(self, recs):
        """Sparse deposition: demotion of lead_group into follow_group plus become_follower(term, 0) on its soft cells and the
        lead-side stop; a DEPOSE_REC_DTYPE array -> HANDOFF_RESP_DTYPE array, positional. Synchronises."""
        recs = np.ascontiguousarray(recs, dtype=DEPOSE_REC_DTYPE)
        resp = np.zeros(len(recs), dtype=HANDOFF_RESP_DTYPE)
        self._check(self.L.rgt_follow_depose(self.h, recs.ctypes.data, len(recs), resp.ctypes.data))
        return resp

    def follow_depose_device(self, events, new_term, lead, out):
        """Dense deposition (asynchronous): events / new_term = the DEVICE columns lead_gate_device wrote, lead = a DEVICE u64
        [follow_stride()] column of lead groups by follow group (HANDOFF_NO_LEAD = none), out as in follow_promote_device."""
        p = self._dev_ptr
        o = HandoffOut(*[p(out.get(k)) for k in HANDOFF_OUT_COLUMNS])
        self._check(self.L.rgt_follow_depose_device(self.h, p(events), p(new_term), p(lead), C.byref(o)))

    def follow_depose_scan_device(self, msg_flags, term, lead, out):
        """The deposition by a new leader's record (asynchronous), in front of follow_step_gated_device with that call's own
        DEVICE columns msg_flags (rg_follow_msgs.flags) and term; lead / out as in follow_depose_device. The soft cells are left
        to the gated step."""
        p = self._dev_ptr
        o = HandoffOut(*[p(out.get(k)) for k in HANDOFF_OUT_COLUMNS])
        self._check(self.L.rgt_follow_depose_scan_device(self.h, p(msg_flags), p(term), p(lead), C.byref(o)))

    # ---- the dense vote step ------------------------------------------------------------------------
    def follow_vote_device(self, msgs, term, from_, out, priority=None, hdr_flags=None, lead=None, answered=None, answered_cap=0, sync=True):
        """rgv_follow_vote_device: MsgRequestVote / MsgRequestPreVote for every followed group in one launch, in front of
        lead_gate_device. msgs / term / from_ = the DEVICE columns of follow_step_gated_device (a request: the flag byte is exactly
        FOLLOW_MSG_VOTE or _PREVOTE); priority = DEVICE i64, hdr_flags = DEVICE u8 (GATE_FORCE), lead = the DEVICE u64 map of
        follow_depose_device, each or None; out = a dict of DEVICE columns status / gate / events (u8) and term / commit / log_term
        (u64); answered = a DEVICE u64 list of answered_cap places or None. sync: -> (requests, grants, rejects, ignored, deposed);
        else asynchronous, the counts are the five device words at follow_vote_counts()."""
        p = self._dev_ptr
        m = self._follow_msgs(msgs)
        o = VoteOut(*[p(out.get(k)) for k in VOTE_OUT_FIELDS[:6]], p(answered), answered_cap)
        counts = (C.c_uint64 * 5)()
        self._check(self.L.rgv_follow_vote_device(self.h, C.byref(m), p(term), p(from_), p(priority), p(hdr_flags), p(lead), C.byref(o),
                                                  counts if sync else None))
        return tuple(int(x) for x in counts) if sync else None

    def follow_vote(self, recs):
        """Sparse vote step: a VOTE_REC_DTYPE array (lead_group = HANDOFF_NO_LEAD where the store does not lead the group) ->
        VOTE_RESP_DTYPE array, positional. Synchronises."""
        recs = np.ascontiguousarray(recs, dtype=VOTE_REC_DTYPE)
        resp = np.zeros(len(recs), dtype=VOTE_RESP_DTYPE)
        self._check(self.L.rgv_follow_vote(self.h, recs.ctypes.data, len(recs), resp.ctypes.data))
        return resp

    def follow_vote_counts(self):
        """Device address of u64 [5]: requests, grants, rejects, ignored, deposed of the last follow_vote_device."""
        return self.L.rgv_follow_vote_counts(self.h)

    # ---- message-at-a-time mirror of RawNode::step -----------------------------------------------
    def set_peers(self, group, peer_ids, term):
        arr = (_u64 * len(peer_ids))(*peer_ids)
        self._check(self.L.rg_set_peers(self.h, group, arr, len(peer_ids), term))

    def step(self, group, from_, term, index, commit=0, reject=False, reject_hint=0, request_snapshot=0,
             ins_full=False, log_term=0):
        m = AppendResponse(from_, term, index, commit, reject_hint, request_snapshot, int(reject), int(ins_full),
                           (C.c_uint8 * 6)(), log_term)
        self._check(self.L.rg_step(self.h, group, C.byref(m)))

    def step_bytes(self, group, data, ins_full=False):
        """RawNode::step on one protobuf-encoded eraftpb::Message (bytes); ins_full: the caller's Inflights::full() for the sender."""
        self._check(self.L.rg_step_bytes(self.h, group, bytes(data), len(data), int(ins_full)))

    def local_append(self, group, new_last_index):
        self._check(self.L.rg_local_append(self.h, group, new_last_index))

    def local_persisted(self, group, index):
        self._check(self.L.rg_local_persisted(self.h, group, index))

    def mark_sent(self, group, peer_id):
        self._check(self.L.rg_mark_sent(self.h, group, peer_id))

    def local_become_leader(self, group, term):
        """Raft::become_leader at `term` for one group, queued like the other leader-local events."""
        self._check(self.L.rg_local_become_leader(self.h, group, term))

    def flush(self):
        self._check(self.L.rg_flush(self.h))

    # ---- multi-GPU: publication of commit indices ---------------------------------------------------
    def comm_init(self, rank, world, unique_id=None, transport=None, ring_ticks=0, overflow_slots=0):
        """rg_comm_init (a collective). unique_id: bytes from comm_unique_id() (RCCL); transport: a Python callable
        (dev_send, dev_recv, bytes_per_rank, hip_stream) -> 0 standing in for the all-gather (tests, other fabrics)."""
        self._comm_keep = []
        cfg = CommConfig(rank, world, None, ALLGATHER_FN(0), None, ring_ticks, overflow_slots)
        if transport is not None:
            cb = ALLGATHER_FN(lambda user, s, r, n, st: int(transport(s, r, n, st) or 0))
            cfg.transport = cb
            self._comm_keep.append(cb)
        else:
            buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
            cfg.unique_id = C.addressof(buf)
            self._comm_keep.append(buf)
        self._check(self.L.rg_comm_init(self.h, C.byref(cfg)))
        self.comm_rank, self.comm_world = rank, world

    def comm_destroy(self):
        self._check(self.L.rg_comm_destroy(self.h))

    def comm_info(self):
        """rg_comm_info_get: rank / world as given, the transport, and -- over RCCL -- the communicator's own ncclCommCount /
        ncclCommUserRank (what proves how many ranks an exchange really spans)."""
        ci = CommInfo()
        self._check(self.L.rg_comm_info_get(self.h, C.byref(ci)))
        return {"rank": ci.rank, "world": ci.world, "transport": TRANSPORT_NAMES.get(ci.transport, str(ci.transport)),
                "in_process": bool(ci.in_process), "rccl_ranks": ci.rccl_ranks, "rccl_rank": ci.rccl_rank}

    def publish_commit(self, full=False):
        self._check(self.L.rg_publish_commit(self.h, PUBLISH_FULL if full else 0))

    def publish_sync(self):
        self._check(self.L.rg_publish_sync(self.h))

    def published_commit(self, rank=None):
        """The replica of `rank`'s commit indices (all ranks: [world][n_groups]) as a host array."""
        ranks = range(self.comm_world) if rank is None else [rank]
        out = np.empty((len(ranks), self.n_groups), dtype=np.uint64)
        for i, r in enumerate(ranks):
            self._check(self.L.rg_published_commit(self.h, r, 0, self.n_groups, out[i].ctypes.data))
        return out if rank is None else out[0]

    def published_commit_ptr(self):
        stride = _u64(0)
        return self.L.rg_published_commit_ptr(self.h, C.byref(stride)), stride.value

    def publish_stats(self):
        st = PublishStats()
        self._check(self.L.rg_publish_stats_get(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in PublishStats._fields_}

    # ---- synthetic stream --------------------------------------------------------------------
    def workload_init(self, workload, seed=0x5EED5EED, first_group=0, fixed_peers=0, sorted_classes=False, group_commit=False):
        w = _Workload(seed, workload, fixed_peers | (WL_PLACE_SORTED if sorted_classes else 0) | (WL_GROUP_COMMIT if group_commit else 0))
        self._check(self.L.rg_workload_init(self.h, C.byref(w), first_group))

    def workload_gen(self, workload, tick, m_index, m_commit, m_hint, m_rs, m_flags, seed=0x5EED5EED, first_group=0,
                     fixed_peers=0, sorted_classes=False, group_commit=False):
        w = _Workload(seed, workload, fixed_peers | (WL_PLACE_SORTED if sorted_classes else 0) | (WL_GROUP_COMMIT if group_commit else 0))
        self._check(self.L.rg_workload_gen(self.h, C.byref(w), first_group, tick, _ptr(m_index), _ptr(m_commit),
                                           _ptr(m_hint), _ptr(m_rs), _ptr(m_flags)))


def _host_state_struct(st):
    return _HostState(st["n_groups"], st["stride"], st["n_slots"], 0,
                      *[st[k].ctypes.data for k in COL.NAMES[:11]])


WL_GROUP_COMMIT = 0x20  # rg_workload.reserved flag: group commit on, three commit groups (RG_WL_GROUP_COMMIT)
WL_PLACE_SORTED = 0x10  # rg_workload.reserved flag: the groups of a shard placed by replica-set size class (RG_WL_PLACE_SORTED)


def workload_init_host(st, workload, seed=0x5EED5EED, first_group=0, fixed_peers=0, sorted_classes=False, group_commit=False):
    """Host twin of Engine.workload_init over numpy columns (no GPU)."""
    L = load_library()
    w = _Workload(seed, workload, fixed_peers | (WL_PLACE_SORTED if sorted_classes else 0) | (WL_GROUP_COMMIT if group_commit else 0))
    s = _host_state_struct(st)
    rc = L.rg_workload_init_host(C.byref(w), first_group, C.byref(s))
    if rc:
        raise EngineError(rc, L.rg_last_error().decode())


def workload_gen_host(st, msgs, workload, tick, seed=0x5EED5EED, first_group=0, fixed_peers=0, sorted_classes=False, group_commit=False):
    """Host twin of Engine.workload_gen: messages of `tick` from the numpy state columns."""
    L = load_library()
    w = _Workload(seed, workload, fixed_peers | (WL_PLACE_SORTED if sorted_classes else 0) | (WL_GROUP_COMMIT if group_commit else 0))
    s = _host_state_struct(st)
    rc = L.rg_workload_gen_host(C.byref(w), first_group, tick, C.byref(s), msgs.m_index.ctypes.data,
                                msgs.m_commit.ctypes.data, msgs.m_hint.ctypes.data, msgs.m_rs.ctypes.data,
                                msgs.m_flags.ctypes.data)
    if rc:
        raise EngineError(rc, L.rg_last_error().decode())


class CommAllConfig(C.Structure):
    _fields_ = [("ring_ticks", C.c_uint32), ("overflow_slots", C.c_uint32), ("transport", C.c_uint32), ("reserved", C.c_uint32)]


COMM_ALL_AUTO, COMM_ALL_RCCL, COMM_ALL_LOCAL = 0, 1, 2
SEND_LAST_IS_TAIL, SEND_LAST_IS_PREV = 0x80000000, 0x40000000


def comm_init_all(engines, ring_ticks=0, overflow_slots=0, transport=COMM_ALL_AUTO):
    """rg_comm_init_all: the engines of ONE process become ranks 0..n-1 of one publication, driven by one thread."""
    L = engines[0].L
    arr = (C.c_void_p * len(engines))(*[e.h for e in engines])
    cfg = CommAllConfig(ring_ticks, overflow_slots, transport, 0)
    engines[0]._check(L.rg_comm_init_all(arr, len(engines), C.byref(cfg)))
    for i, e in enumerate(engines):
        e.comm_rank, e.comm_world = i, len(engines)


def publish_commit_all(engines, full=False):
    """rg_publish_commit_all: one publication of every rank (the n exchanges issued together)."""
    L = engines[0].L
    arr = (C.c_void_p * len(engines))(*[e.h for e in engines])
    engines[0]._check(L.rg_publish_commit_all(arr, len(engines), PUBLISH_FULL if full else 0))


def plan_placement(cfg_words, n_slots):
    """rg_plan_placement (pure host arithmetic): -> (perm u64[G] with perm[i] = current position of the group that goes to
    position i, [(first_group, n_groups, n_slots)] = the ranges the engine will derive from the permuted column)."""
    L = load_library()
    cfg = np.ascontiguousarray(cfg_words, dtype=np.uint32)
    perm = np.zeros(len(cfg), dtype=np.uint64)
    dt = np.dtype([("first_group", "<u8"), ("n_groups", "<u8"), ("n_slots", "<u4"), ("reserved", "<u4")])
    out = np.zeros(16, dtype=dt)
    n = C.c_uint32(0)
    rc = L.rg_plan_placement(cfg.ctypes.data, len(cfg), n_slots, perm.ctypes.data, out.ctypes.data, len(out), C.byref(n))
    if rc:
        raise EngineError(rc, L.rg_last_error().decode())
    return perm, [(int(r["first_group"]), int(r["n_groups"]), int(r["n_slots"])) for r in out[:min(n.value, len(out))]]


def comm_warmup():
    """rg_comm_warmup: load RCCL and run a one-rank communicator through its life on the current device (start-up cost, paid early)."""
    L = load_library()
    rc = L.rg_comm_warmup()
    if rc:
        raise EngineError(rc, L.rg_last_error().decode())


def comm_unique_id():
    """rg_comm_unique_id: the RCCL unique id rank 0 hands to the other ranks (128 bytes)."""
    L = load_library()
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    rc = L.rg_comm_unique_id(buf)
    if rc:
        raise EngineError(rc, L.rg_last_error().decode())
    return bytes(buf)


def pub_bytes_per_rank(n_groups, overflow_slots=0):
    return load_library().rg_pub_bytes_per_rank(n_groups, overflow_slots)


def pub_accumulate_host(old_commit, new_commit, slice_, overflow_slots=0):
    """Host twin of the ticks' publication byte: accumulate old -> new into `slice_` (uint8 array, in place)."""
    L = load_library()
    a, b = np.ascontiguousarray(old_commit, dtype=np.uint64), np.ascontiguousarray(new_commit, dtype=np.uint64)
    rc = L.rg_pub_accumulate_host(len(a), overflow_slots, a.ctypes.data, b.ctypes.data, slice_.ctypes.data)
    if rc:
        raise EngineError(rc, L.rg_last_error().decode())


def pub_apply_host(n_groups, world, gathered, replica, overflow_slots=0):
    """Host twin of the replica update: add one gathered publication to `replica` ([world][stride]). Returns the
    number of slices that ask for a full resynchronisation."""
    L = load_library()
    lost = C.c_uint32(0)
    rc = L.rg_pub_apply_host(n_groups, overflow_slots, world, gathered.ctypes.data, replica.ctypes.data, C.byref(lost))
    if rc:
        raise EngineError(rc, L.rg_last_error().decode())
    return lost.value


def decode_message(data):
    """rg_decode_message: the decoder behind rg_step_bytes alone (pure host code). Returns a dict of the fields."""
    m = DecodedMessage()
    L = load_library()
    rc = L.rg_decode_message(bytes(data), len(data), C.byref(m))
    if rc != 0:
        raise EngineError(rc, L.rg_last_error().decode())
    return {k.rstrip("_"): int(getattr(m, k)) for k, _ in DecodedMessage._fields_}


def _entries_c(entries):
    """[{entry_type, term, index, data, context, sync_log}] -> (EntryC array, keep-alive list)."""
    arr = (EntryC * max(1, len(entries)))()
    keep = []
    for a, e in zip(arr, entries):
        d, c = bytes(e.get("data", b"")), bytes(e.get("context", b""))
        keep += [d, c]
        a.entry_type, a.sync_log = int(e.get("entry_type", 0)), int(bool(e.get("sync_log", False)))
        a.term, a.index = int(e.get("term", 0)), int(e.get("index", 0))
        a.data, a.data_len, a.context, a.context_len = (d or None), len(d), (c or None), len(c)
    return arr, keep


def entry_size(entry):
    """rg_entry_size: Entry::compute_size()."""
    arr, _keep = _entries_c([entry])
    return int(load_library().rg_entry_size(arr))


def limit_size(entries, max_size):
    """rg_limit_size: how many of `entries` one message keeps under util::limit_size(max_size) (None = NO_LIMIT)."""
    arr, _keep = _entries_c(entries)
    return int(load_library().rg_limit_size(arr, len(entries), (1 << 64) - 1 if max_size is None else int(max_size)))


def encode_message(fields, entries=(), snapshot=None, context=b"", cap=None):
    """rg_encode_message: an outgoing eraftpb::Message -> bytes. `fields`: the scalar fields by their .proto names;
    `snapshot`: an already serialised eraftpb::Snapshot or None; `cap`: buffer size to offer (default: exactly enough)."""
    L = load_library()
    arr, _keep = _entries_c(list(entries))
    m = MessageC()
    for k, v in fields.items():
        setattr(m, "from_" if k == "from" else k, int(v))
    m.entries, m.n_entries = arr, len(entries)
    ctx = bytes(context)
    m.context, m.context_len = (ctx or None), len(ctx)
    if snapshot is not None:
        snap = bytes(snapshot)
        # (c_char_p(b"") is a valid non-NULL pointer: a present, empty Snapshot)
        m.snapshot, m.snapshot_len = snap, len(snap)
    n = C.c_uint64(0)
    rc = L.rg_message_size(C.byref(m), C.byref(n))
    if rc != 0:
        raise EngineError(rc, L.rg_last_error().decode())
    size = n.value if cap is None else int(cap)
    buf = C.create_string_buffer(max(1, size))
    rc = L.rg_encode_message(C.byref(m), buf, size, C.byref(n))
    if rc != 0:
        raise EngineError(rc, L.rg_last_error().decode())
    return buf.raw[:n.value]
