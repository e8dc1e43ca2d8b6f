#!/usr/bin/env python3
"""Generate the Rust FFI bindings of include/raftgroups.h and of its extension headers include/raftgroups_lead.h,
include/raftgroups_term.h, include/raftgroups_vote.h, include/raftgroups_handoff.h, include/raftgroups_conf.h,
include/raftgroups_transfer.h and include/raftgroups_mirror.h.

    python tools/gen_rust_bindings.py            # writes bindings/raftgroups.rs, bindings/raftgroups_lead.rs, bindings/raftgroups_term.rs, bindings/raftgroups_vote.rs, bindings/raftgroups_handoff.rs, bindings/raftgroups_conf.rs, bindings/raftgroups_transfer.rs, bindings/raftgroups_mirror.rs and the block in INTEGRATION.md
    python tools/gen_rust_bindings.py --check    # exit 1 if any of them is out of date (tests/test_abi.py runs this)

Everything is derived from the header: `#[repr(C)]` structs, the `extern "C"` block (one declaration per exported
function, same argument order), the numeric constants. No Rust toolchain exists in the build image, so the output is
source a maintainer compiles on their side; what IS checked here is that it names every export of libraftgroups.so with
the header's arity (tests/test_abi.py).
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "raftgroups.h")
OUT_RS = os.path.join(ROOT, "bindings", "raftgroups.rs")
LEAD_HEADER = os.path.join(ROOT, "include", "raftgroups_lead.h")  # the extension: rgx_* functions, RG_* / RGX_* constants
LEAD_RS = os.path.join(ROOT, "bindings", "raftgroups_lead.rs")
TERM_HEADER = os.path.join(ROOT, "include", "raftgroups_term.h")  # the second extension: rgt_* functions and types, RGT_* constants
TERM_RS = os.path.join(ROOT, "bindings", "raftgroups_term.rs")
VOTE_HEADER = os.path.join(ROOT, "include", "raftgroups_vote.h")  # the third extension: rgv_* functions and types, RGV_* constants
VOTE_RS = os.path.join(ROOT, "bindings", "raftgroups_vote.rs")
HANDOFF_HEADER = os.path.join(ROOT, "include", "raftgroups_handoff.h")  # the fourth extension: rgh_* functions and types, RGH_* constants
HANDOFF_RS = os.path.join(ROOT, "bindings", "raftgroups_handoff.rs")
CONF_HEADER = os.path.join(ROOT, "include", "raftgroups_conf.h")  # the fifth extension: rgc_* functions and types, RGC_* constants
CONF_RS = os.path.join(ROOT, "bindings", "raftgroups_conf.rs")
TRANSFER_HEADER = os.path.join(ROOT, "include", "raftgroups_transfer.h")  # the sixth extension: rgm_* functions and types, RGM_* constants
TRANSFER_RS = os.path.join(ROOT, "bindings", "raftgroups_transfer.rs")
MIRROR_HEADER = os.path.join(ROOT, "include", "raftgroups_mirror.h")  # the seventh extension: rgr_* functions and types, RGR_* constants
MIRROR_RS = os.path.join(ROOT, "bindings", "raftgroups_mirror.rs")
DOC = os.path.join(ROOT, "INTEGRATION.md")
BEGIN, END = "<!-- BEGIN GENERATED: tools/gen_rust_bindings.py -->", "<!-- END GENERATED -->"

SCALARS = {"uint64_t": "u64", "uint32_t": "u32", "uint16_t": "u16", "uint8_t": "u8", "int32_t": "i32", "int64_t": "i64",
           "int": "i32", "unsigned": "u32", "double": "f64", "float": "f32", "size_t": "usize", "char": "c_char", "void": "c_void"}
KEYWORDS = {"match", "type", "ref", "box", "move", "fn", "in", "loop", "self", "use", "mod", "as", "where"}


def strip_comments(src):
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def camel(name):
    return "".join(p.capitalize() for p in name.split("_"))


def rust_type(ctype, typedefs):
    """ctype: e.g. 'const uint64_t *', 'rg_engine **', 'void *'."""
    # `base q0 * q1 * q2 ...`: q0 qualifies the pointee of the innermost pointer, q_k (k >= 1) the k-th pointer itself -- i.e.
    # the pointee of the (k+1)-th. `rg_engine *const *engines` is a pointer to CONST pointers to mutable engines:
    # *const *mut RgEngine (round 5's generator had the two levels swapped).
    parts = ctype.strip().split("*")
    stars = len(parts) - 1
    consts = [bool(re.search(r"\bconst\b", q)) for q in parts]
    base = re.sub(r"\bconst\b|\bstruct\b", " ", parts[0]).strip()
    if base in SCALARS:
        r = SCALARS[base]
    elif base in typedefs:
        r = typedefs[base]
    else:
        raise ValueError(f"unknown C type {ctype!r}")
    for k in range(stars):
        r = ("*const " if consts[k] else "*mut ") + r
    return r


def ident(name):
    return "r#" + name if name in KEYWORDS else name


def parse_decl(decl, typedefs, as_param):
    """'const uint64_t *peer_ids' / 'uint64_t match[RG_MAX_SLOTS]' -> (name, rust type)."""
    decl = decl.strip()
    m = re.match(r"^(.*?)(\w+)\s*(\[\s*(\w+)\s*\])?$", decl, flags=re.S)
    if not m:
        raise ValueError(decl)
    ctype, name, arr, n = m.group(1), m.group(2), m.group(3), m.group(4)
    if not ctype.strip():  # unnamed parameter such as 'void'
        ctype, name = name, ""
    rt = rust_type(ctype, typedefs)
    if arr:
        if as_param:  # arrays decay to pointers
            rt = ("*const " if "const" in ctype else "*mut ") + rt
        else:
            rt = f"[{rt}; {n + ' as usize' if not n.isdigit() else int(n)}]"
    return name, rt


def parse(src, fn_prefix="rg_", known=None, const_prefix="RGX?_"):
    """fn_prefix: the prefix of the header's functions; known: typedefs of a header this one includes (the extension);
    const_prefix: a regular expression for the prefix of the header's constants."""
    src = strip_comments(src)
    consts, structs, funcs, enums = [], [], [], []
    typedefs = {"rg_engine": "RgEngine"}
    typedefs.update(known or {})
    for m in re.finditer(r"^[ \t]*#define[ \t]+(" + const_prefix + r"\w+)[ \t]+(\(?-?(?:0x[0-9a-fA-F]+|\d+)(?:u|U|ull|ULL)?\)?)[ \t]*$", src, flags=re.M):
        v = m.group(2).strip("()")
        wide = v.lower().endswith("ull")
        v = re.sub(r"(?i)u?l*$", "", v)
        consts.append((m.group(1), v, "u64" if wide else "u32"))
    for m in re.finditer(r"typedef\s+enum\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
        items, nxt = [], 0
        for it in m.group(1).split(","):
            it = it.strip()
            if not it:
                continue
            if "=" in it:
                k, v = [x.strip() for x in it.split("=")]
                nxt = int(v, 0)
            else:
                k = it
            items.append((k, nxt))
            nxt += 1
        enums.append((m.group(2), items))
        typedefs[m.group(2)] = "i32"
    fp = re.search(r"typedef\s+(\w+)\s*\(\s*\*\s*(\w+)\s*\)\s*\((.*?)\)\s*;", src, flags=re.S)
    fnptr = None
    if fp:
        fnptr = (fp.group(2), fp.group(1), fp.group(3))
        typedefs[fp.group(2)] = camel(fp.group(2))
    for m in re.finditer(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
        typedefs[m.group(2)] = camel(m.group(2))
    for m in re.finditer(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
        fields = []
        for stmt in m.group(1).split(";"):
            stmt = " ".join(stmt.split())
            if not stmt:
                continue
            # 'uint64_t a, b' / 'uint64_t *m, *n' / 'uint64_t m[8], n[8]': several declarators share the base type, each
            # brings its own stars and array bounds
            bm = re.match(r"^((?:const\s+)?(?:struct\s+)?\w+)\s*(.*)$", stmt)
            base, decls = bm.group(1), bm.group(2)
            for d in decls.split(","):
                fields.append(parse_decl(base + " " + d.strip(), typedefs, False))
        structs.append((m.group(2), fields))
    body = re.sub(r"typedef\s+(struct|enum)\s*\{.*?\}\s*\w+\s*;", " ", src, flags=re.S)
    body = re.sub(r"typedef[^;{]*;", " ", body)
    body = re.sub(r"^[ \t]*#.*$", " ", body, flags=re.M)
    for m in re.finditer(r"([\w \t\*]+?)\b(" + fn_prefix + r"\w+)\s*\(([^()]*)\)\s*;", body, flags=re.S):
        ret, name, args = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
        params = []
        if args and args != "void":
            for a in args.split(","):
                params.append(parse_decl(a, typedefs, True))
        funcs.append((name, None if ret == "void" else rust_type(ret, typedefs), params))
    if fnptr:
        name, ret, args = fnptr
        ps = [parse_decl(a, typedefs, True) for a in " ".join(args.split()).split(",")]
        fnptr = (camel(name), rust_type(ret, typedefs), ps)
    return consts, enums, structs, funcs, fnptr


def emit(consts, enums, structs, funcs, fnptr):
    o = ["// GENERATED from include/raftgroups.h by tools/gen_rust_bindings.py -- do not edit.",
         "// Link with `-lraftgroups` (build.rs: cargo:rustc-link-lib=dylib=raftgroups). Never compiled in the build image (no",
         "// Rust toolchain there); tests/test_abi.py checks that it names every export of libraftgroups.so with the header's arity.",
         "#![allow(non_camel_case_types, dead_code)]",
         "use std::os::raw::{c_char, c_void};", ""]
    for name, v, ty in consts:
        o.append(f"pub const {name}: {ty} = {v};")
    o.append("")
    for ename, items in enums:
        o.append(f"// {ename}")
        for k, v in items:
            o.append(f"pub const {k}: i32 = {v};")
        o.append("")
    o.append("pub enum RgEngine {} // opaque")
    if fnptr:
        n, ret, ps = fnptr
        o.append(f"pub type {n} = Option<unsafe extern \"C\" fn({', '.join(t for _, t in ps)}) -> {ret}>;")
    o.append("")
    for sname, fields in structs:
        o.append("#[repr(C)]")
        o.append(f"pub struct {camel(sname)} {{")
        for fname, ft in fields:
            o.append(f"    pub {ident(fname)}: {ft},")
        o.append("}")
        o.append("")
    o.append('extern "C" {')
    for name, ret, params in funcs:
        ps = ", ".join(f"{ident(n) if n else '_'}: {t}" for n, t in params)
        o.append(f"    pub fn {name}({ps})" + (f" -> {ret}" if ret else "") + ";")
    o.append("}")
    o += ["",
          "/// Error mapping back to raft::Error (src/errors.rs:6-50)",
          "pub fn check(rc: i32) -> raft::Result<()> {",
          "    match rc {",
          "        0 => Ok(()),",
          "        RG_ERR_STEP_LOCAL_MSG => Err(raft::Error::StepLocalMsg),",
          "        RG_ERR_STEP_PEER_NOT_FOUND => Err(raft::Error::StepPeerNotFound), // checked BEFORE the term, as RawNode::step does",
          "        _ => panic!(\"raftgroups: {}\", unsafe { std::ffi::CStr::from_ptr(rg_last_error()) }.to_string_lossy()),",
          "    }",
          "}", ""]
    return "\n".join(o)


def generate():
    return emit(*parse(open(HEADER, encoding="utf-8").read()))


def struct_names(path):
    src = strip_comments(open(path, encoding="utf-8").read())
    return {m.group(2): camel(m.group(2)) for m in re.finditer(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S)}


def generate_extension(header, fn_prefix, const_prefix, below, what, checked_by, extra_consts=()):
    """The bindings of one extension header: its constants, structs and functions, over the types of the headers `below` it
    (their generated modules are `use`d). what / checked_by: the two comment lines under the GENERATED line."""
    known = {}
    for h in below:
        known.update(struct_names(h))
    consts, _, structs, funcs, _ = parse(open(header, encoding="utf-8").read(), fn_prefix=fn_prefix, known=known, const_prefix=const_prefix)
    o = ["// GENERATED from include/%s by tools/gen_rust_bindings.py -- do not edit." % os.path.basename(header), what, checked_by,
         "#![allow(non_camel_case_types, dead_code)]"]
    o += ["use super::%s::*;" % os.path.splitext(os.path.basename(h))[0] for h in below] + [""]
    for name, v, ty in consts:
        o.append(f"pub const {name}: {ty} = {v};")
    o += list(extra_consts) + [""]
    for sname, fields in structs:
        o += ["#[repr(C)]", f"pub struct {camel(sname)} {{"] + [f"    pub {ident(fname)}: {ft}," for fname, ft in fields] + ["}", ""]
    if funcs:  # (a header may declare objects only: extra_consts carries those)
        o.append('extern "C" {')
        for name, ret, params in funcs:
            ps = ", ".join(f"{ident(n) if n else '_'}: {t}" for n, t in params)
            o.append(f"    pub fn {name}({ps})" + (f" -> {ret}" if ret else "") + ";")
        o += ["}", ""]
    return "\n".join(o)


def generate_lead():
    """bindings/raftgroups_lead.rs: the extension header's constants, structs and rgx_* functions, over the core module's types."""
    return generate_extension(LEAD_HEADER, "rgx_", "RGX?_", [HEADER],
                              "// The leader's clock, an extension of raftgroups.rs (same library). tests/test_lead_clock_host.py checks that it names every",
                              "// rgx_* export of libraftgroups.so with the header's arity.", ["pub const RG_HANDOFF_NO_LEAD: u64 = u64::MAX;"])


def generate_term():
    """bindings/raftgroups_term.rs: the second extension header's constants, structs and rgt_* functions, over the types of the
    core module and of the first extension."""
    return generate_extension(TERM_HEADER, "rgt_", "RGT_", [HEADER, LEAD_HEADER],
                              "// The leader's term gate and the deposition, an extension of raftgroups.rs and raftgroups_lead.rs (same library).",
                              "// tests/test_term_gate_host.py checks that it names every rgt_* export of libraftgroups.so with the header's arity.")


def generate_vote():
    """bindings/raftgroups_vote.rs: the third extension header's constants, structs and rgv_* functions, over the types of the
    core module and of the two extensions before it."""
    return generate_extension(VOTE_HEADER, "rgv_", "RGV_", [HEADER, LEAD_HEADER, TERM_HEADER],
                              "// The dense vote step, an extension of raftgroups.rs, raftgroups_lead.rs and raftgroups_term.rs (same library).",
                              "// tests/test_vote_step_host.py checks that it names every rgv_* export of libraftgroups.so with the header's arity.")


def generate_handoff():
    """bindings/raftgroups_handoff.rs: the fourth extension header's constants, structs and rgh_* functions, over the core module's
    types (the header includes raftgroups.h alone)."""
    return generate_extension(HANDOFF_HEADER, "rgh_", "RGH_", [HEADER],
                              "// The promotion into an engine with device Inflights, an extension of raftgroups.rs (same library).",
                              "// tests/test_promote_send_host.py checks that it names every rgh_* export of libraftgroups.so with the header's arity.")


def generate_conf():
    """bindings/raftgroups_conf.rs: the fifth extension header's constants, structs and rgc_* functions, over the core module's
    types (the header includes raftgroups.h alone)."""
    return generate_extension(CONF_HEADER, "rgc_", "RGC_", [HEADER],
                              "// The batched conf change (apply_conf and post_conf_change on the device), an extension of raftgroups.rs (same library).",
                              "// tests/test_conf_change_host.py checks that it names every rgc_* export of libraftgroups.so with the header's arity.")


def generate_transfer():
    """bindings/raftgroups_transfer.rs: the sixth extension header's constants, structs and rgm_* functions, over the core module's
    types (the header includes raftgroups.h alone)."""
    return generate_extension(TRANSFER_HEADER, "rgm_", "RGM_", [HEADER],
                              "// The batched leader transfer (handle_transfer_leader on the device), an extension of raftgroups.rs (same library).",
                              "// tests/test_transfer_host.py checks that it names every rgm_* export of libraftgroups.so with the header's arity.")


def generate_mirror():
    """bindings/raftgroups_mirror.rs: the seventh extension header's constants, structs and rgr_* functions, over the core module's
    types (the header includes raftgroups.h alone)."""
    return generate_extension(MIRROR_HEADER, "rgr_", "RGR_", [HEADER],
                              "// The dense tick's read mirror (its counters), an extension of raftgroups.rs (same library).",
                              "// tests/test_mirror_host.py checks that it names the rgr_* export of libraftgroups.so -- an OBJECT holding the function's address.",
                              ['', 'extern "C" {', '    pub static rgr_mirror_stats: unsafe extern "C" fn(h: *const RgEngine, info: *mut RgrMirrorInfo) -> i32;', '}'])


def doc_with_block(doc, rs):
    block = f"{BEGIN}\n```rust\n{rs}```\n{END}"
    if BEGIN in doc and END in doc:
        return doc[:doc.index(BEGIN)] + block + doc[doc.index(END) + len(END):]
    raise SystemExit("INTEGRATION.md lacks the generated-block markers")


def main():
    rs, lead_rs, term_rs, vote_rs, handoff_rs, conf_rs = generate(), generate_lead(), generate_term(), generate_vote(), generate_handoff(), generate_conf()
    transfer_rs = generate_transfer()
    mirror_rs = generate_mirror()
    doc = open(DOC, encoding="utf-8").read()
    new_doc = doc_with_block(doc, rs)
    if "--check" in sys.argv:
        stale = []
        if not os.path.exists(OUT_RS) or open(OUT_RS, encoding="utf-8").read() != rs:
            stale.append(OUT_RS)
        if not os.path.exists(LEAD_RS) or open(LEAD_RS, encoding="utf-8").read() != lead_rs:
            stale.append(LEAD_RS)
        if not os.path.exists(TERM_RS) or open(TERM_RS, encoding="utf-8").read() != term_rs:
            stale.append(TERM_RS)
        if not os.path.exists(VOTE_RS) or open(VOTE_RS, encoding="utf-8").read() != vote_rs:
            stale.append(VOTE_RS)
        if not os.path.exists(HANDOFF_RS) or open(HANDOFF_RS, encoding="utf-8").read() != handoff_rs:
            stale.append(HANDOFF_RS)
        if not os.path.exists(CONF_RS) or open(CONF_RS, encoding="utf-8").read() != conf_rs:
            stale.append(CONF_RS)
        if not os.path.exists(TRANSFER_RS) or open(TRANSFER_RS, encoding="utf-8").read() != transfer_rs:
            stale.append(TRANSFER_RS)
        if not os.path.exists(MIRROR_RS) or open(MIRROR_RS, encoding="utf-8").read() != mirror_rs:
            stale.append(MIRROR_RS)
        if new_doc != doc:
            stale.append(DOC)
        if stale:
            print("out of date (run tools/gen_rust_bindings.py):", ", ".join(stale))
            return 1
        return 0
    os.makedirs(os.path.dirname(OUT_RS), exist_ok=True)
    open(OUT_RS, "w", encoding="utf-8").write(rs)
    open(LEAD_RS, "w", encoding="utf-8").write(lead_rs)
    open(TERM_RS, "w", encoding="utf-8").write(term_rs)
    open(VOTE_RS, "w", encoding="utf-8").write(vote_rs)
    open(HANDOFF_RS, "w", encoding="utf-8").write(handoff_rs)
    open(CONF_RS, "w", encoding="utf-8").write(conf_rs)
    open(TRANSFER_RS, "w", encoding="utf-8").write(transfer_rs)
    open(MIRROR_RS, "w", encoding="utf-8").write(mirror_rs)
    open(DOC, "w", encoding="utf-8").write(new_doc)
    print(f"wrote {OUT_RS}, {LEAD_RS}, {TERM_RS}, {VOTE_RS}, {HANDOFF_RS}, {CONF_RS}, {TRANSFER_RS}, {MIRROR_RS} and the generated block of {DOC}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
