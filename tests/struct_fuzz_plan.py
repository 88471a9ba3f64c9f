"""Host half of the struct-hashing fuzz (test_gpu_struct_fuzz.py): record
layouts beyond the flat grammar -- nested structs, []byte slots and list fields
(MK_FIELD_STRUCT / VARBYTES / LIST, include/prysm_merkle.h) -- their records,
the resident lives and the tree sets over them, and the coverage they reach,
drawn from seeded streams without a device.  test_struct_fuzz_host.py checks
this plan on the CPU; the GPU test runs exactly the same plan.

A layout is an oracle type tuple (oracle/ssz_ref.py) and the capacities of its
slices and []byte fields, laid out by struct_list_ref.flatten.  Random layouts
are drawn inside the header's limits (32 entries, depth 4, 256 chunks per list,
the column bytes of the workgroup forms), directed ones name the branch they
are there for, and a third group is padded with raw fields until its column
peak sits exactly on or 4 bytes above a workgroup-size switch.  column_bytes()
restates the header's rule for the column; nothing here asks the library.

Sizes: a record stays at or below 16 KB, a layout's records at or below
RECORDS_BYTES in all, a resident tree at or below 512 records."""
import os
import random
from collections import Counter
from functools import lru_cache

import numpy as np

from tests import struct_list_ref as SL
from tests import tree_fuzz_plan as TP
from tests.struct_list_ref import BYTES, LIST, RAW, STRUCT, VARBYTES

# PRYSM_FUZZ_SEED shifts every stream, PRYSM_FUZZ_SCALE multiplies the number of
# random layouts (as in test_gpu_fuzz.py).  The coverage conditions are asserted
# for the committed run, PRYSM_FUZZ_SEED unset or 0.
FUZZ_SEED = int(os.environ.get("PRYSM_FUZZ_SEED", "0"))
SEED = 0x5EED000000000000 + 9700 + 1000 * FUZZ_SEED
SCALE = max(1, int(os.environ.get("PRYSM_FUZZ_SCALE", "1")))

BYTEARRAY_LENS = [1, 4, 20, 32, 33, 48, 96, 124, 128, 131, 132, 133, 136, 200]
SLOT_SIZES = [0, 8, 64, 127, 128, 131, 132, 133, 140, 200]
ITEM_BYTEARRAY_LENS = [4, 32, 48, 96, 128, 132, 136]
RECORD_COUNTS = [1, 2, 63, 64, 65, 129, 257]
VAR_LENGTHS = [0, "cap", 131, 132, 133]
COUNT_TAGS = ["0", "1", "ipc-1", "ipc", "ipc+1", "2ipc", "2ipc+1", "cap"]

MAX_ENTRIES, MAX_DEPTH, MAX_CHUNKS, MAX_RECORD = 32, 4, 256, 16 * 1024
RECORDS_BYTES = 96 * 1024   # per layout: keeps the two references to seconds over the whole plan
LIST_BYTES = 4096           # the cells of one random list
NESTED_SWITCH, NESTED_LIMIT = 160, 320   # k_struct_nested: 256 threads up to the switch, 128 up to the limit
LIST_SWITCH, LIST_LIMIT = 320, 640       # k_struct_list: 128 threads up to the switch, 64 up to the limit
FORMS = ["flat", "nested256", "nested128", "list128", "list64"]

RANDOM_LAYOUTS = {"flat": 6, "nested": 44, "list": 50, "list128": 8}   # test_gpu_struct_fuzz.py's docstring has the measured times
PEAK_LAYOUTS = 5            # per aimed peak
TREE_SETS = 10
LIFE_STEPS = ["update", "append", "erase", "truncate", "clone_diverge", "copy_from", "reserve", "audit", "diff",
              "branches"]
LIFE_CAP = 512

U8, U16, U32, U64, BOOL, BY = ("uint", 8), ("uint", 16), ("uint", 32), ("uint", 64), ("bool",), ("bytes",)
SCALARS = [U8, U16, U32, U64, BOOL]


def BA(n):
    return ("bytearray", n)


def _align4(x):
    return (x + 3) & ~3


# ---- the header's rules, restated ------------------------------------------------------------------
def _out(entry):
    return entry[2] if entry[0] == RAW else 32


def stack_levels(chunks):
    """Levels of a list's node stack: 0 for one chunk, else the bit length of ceil(chunks / 2)."""
    return 0 if chunks <= 1 else ((chunks + 1) // 2).bit_length()


def list_chunks(fields, f, count=None):
    ikind, _, ilen = fields[f + 1]
    ipc = 128 // (ilen if ikind == RAW else 32)
    return -(-(fields[f][2] if count is None else count) // ipc)


def msg_len(fields, f0, f1):
    """Message length of the struct whose direct children are entries [f0, f1)."""
    own, f = 0, f0
    while f < f1:
        own += _out(fields[f])
        f += SL._span(fields, f)
    return own


def column_bytes(fields):
    """Column bytes a record needs along its longest nesting path, by the
    header's text: every message length rounded up to 4, 256 B for a list's
    chunk pair, 32 B per level of its node stack, a struct item's messages
    behind those.  A struct's region starts behind its parent's whole message."""
    def walk(f0, f1, base):
        behind = base + _align4(msg_len(fields, f0, f1))
        peak, f = behind, f0
        while f < f1:
            kind, _, ln = fields[f]
            if kind == STRUCT:
                peak = max(peak, walk(f + 1, f + 1 + ln, behind))
            elif kind == LIST:
                after = behind + 256 + 32 * stack_levels(list_chunks(fields, f))
                peak = max(peak, after)
                if fields[f + 1][0] == STRUCT:
                    peak = max(peak, walk(f + 2, f + 2 + fields[f + 1][2], after))
            f += SL._span(fields, f)
        return peak
    return walk(0, len(fields), 0)


def entries_of(fields):
    """(f, depth, place) of every entry: depth of the struct that holds it (the
    top-level struct is 1), place 'top' | 'nested' | 'item' (a list's item
    descriptor) | 'in_item' (a field of a struct item)."""
    out = []

    def walk(f0, f1, depth, in_item):
        f = f0
        while f < f1:
            kind, _, ln = fields[f]
            out.append((f, depth, "in_item" if in_item else "top" if depth == 1 else "nested"))
            if kind == STRUCT:
                walk(f + 1, f + 1 + ln, depth + 1, in_item)
            elif kind == LIST:
                out.append((f + 1, depth, "item"))
                if fields[f + 1][0] == STRUCT:
                    walk(f + 2, f + 2 + fields[f + 1][2], depth + 1, True)
            f += SL._span(fields, f)
    walk(0, len(fields), 1, False)
    return out


def struct_depth(fields):
    """Deepest struct, the top-level one counting as 1 and an item struct as one level."""
    return max([1] + [d + 1 for f, d, _ in entries_of(fields) if fields[f][0] == STRUCT])


def verdict(fields, rec_len):
    """(form, why): the form the header promises for the layout, or None and the limit it breaks."""
    kinds = {k for k, _, _ in fields}
    if len(fields) > MAX_ENTRIES:
        return None, "more than 32 entries"
    if struct_depth(fields) > MAX_DEPTH:
        return None, "deeper than 4"
    if any(k == LIST and list_chunks(fields, f) > MAX_CHUNKS for f, (k, _, _) in enumerate(fields)):
        return None, "more than 256 chunks"
    peak = column_bytes(fields)
    if LIST in kinds:
        if peak > LIST_LIMIT:
            return None, f"column {peak} B above {LIST_LIMIT}"
        return ("list128" if peak <= LIST_SWITCH else "list64"), None
    if STRUCT in kinds or VARBYTES in kinds:
        if peak > NESTED_LIMIT:
            return None, f"column {peak} B above {NESTED_LIMIT}"
        return ("nested256" if peak <= NESTED_SWITCH else "nested128"), None
    return "flat", None


def scratch_bytes(fields):
    """What mk_ssz_struct_msg_len returns for an accepted layout: the top-level
    message length; with MK_FIELD_STRUCT entries the message lengths of the
    top-level struct and of every nested struct summed."""
    top = msg_len(fields, 0, len(fields))
    subs = [msg_len(fields, f + 1, f + 1 + ln) for f, (k, _, ln) in enumerate(fields) if k == STRUCT]
    return top + sum(subs)


# ---- random types ------------------------------------------------------------------------------------
class _Budget:
    def __init__(self, entries, list_bytes):
        self.entries, self.list_bytes = entries, list_bytes


def _list_cap(rng, ipc):
    return max(1, rng.choice([1, ipc - 1, ipc, ipc + 1, 2 * ipc, 2 * ipc + 1, 5 * ipc + 3, rng.randint(1, 40 * ipc),
                              rng.randint(1, 40 * ipc)]))


def _gen_struct(rng, tag, depth, room, bud, caps, kind, in_item=False):
    """A struct type at nesting depth ``depth`` whose messages, and those behind
    it, fit ``room`` column bytes; its capacities are appended to ``caps`` in
    declaration order.  kind: 'flat' | 'nested' | 'list'."""
    want = min(rng.randint(1, 6), bud.entries, max(1, room // 32 if room < 192 else 6))
    draws = []
    for _ in range(max(want, 1)):
        r = rng.random()
        if kind == "flat":
            draws.append("raw" if r < 0.5 else "ba")
        elif r < 0.30:
            draws.append("raw")
        elif r < 0.48:
            draws.append("ba")
        elif r < 0.66:
            draws.append("by")
        elif r < 0.84 or kind != "list" or in_item:
            draws.append("st")
        else:
            draws.append("ls")
    scal = [rng.choice(SCALARS) for _ in draws]
    own = lambda: sum((1 if s == BOOL else s[1] // 8) if d == "raw" else 32 for d, s in zip(draws, scal))
    while len(draws) > 1 and _align4(own()) > room:
        draws.pop(), scal.pop()
    if _align4(own()) > room:  # a single field of 32 B where fewer are left
        draws, scal = ["raw"], [U8 if room < 8 else U64]
    bud.entries -= len(draws)
    rest = room - _align4(own())
    fields = []
    for i, (d, s) in enumerate(zip(draws, scal)):
        name = f"F{i}"
        if d == "st" and (depth == MAX_DEPTH or rest < 4 or bud.entries < 1):
            d = "ba"
        if d == "ls" and (rest < 256 or bud.entries < 1 or bud.list_bytes < 64):
            d = "ba"
        if d == "raw":
            ft = s
        elif d == "ba":
            ft = BA(rng.choice(BYTEARRAY_LENS))
        elif d == "by":
            ft = BY
            caps.append(rng.choice(SLOT_SIZES))
        elif d == "st":
            sub = ("struct", f"{tag}{i}", _gen_struct(rng, f"{tag}{i}_", depth + 1, rest, bud, caps, kind, in_item))
            ft = ("ptr", sub) if rng.random() < 0.5 else sub
        else:
            ft = ("slice", _gen_item(rng, f"{tag}{i}", depth, rest, bud, caps))
        fields.append((name, ft))
    return fields


def _gen_item(rng, tag, depth, rest, bud, caps):
    """The item type of a list in a struct of depth ``depth`` with ``rest``
    column bytes behind its parent's message; appends the list's capacity,
    then the item's own capacities."""
    bud.entries -= 1  # the item descriptor
    at = len(caps)
    caps.append(None)
    max_levels = (rest - 256) // 32
    r = rng.random()
    if r < 0.4 or (r >= 0.65 and (depth == MAX_DEPTH or bud.entries < 1 or rest < 256 + 8)):
        item = rng.choice(SCALARS)
        stride = ipc_out = 1 if item == BOOL else item[1] // 8
        ipc = 128 // ipc_out
    elif r < 0.65:
        item = BA(rng.choice(ITEM_BYTEARRAY_LENS))
        stride, ipc = item[1], 4
    else:
        item, ipc, stride = None, 4, None
    cap = _list_cap(rng, ipc)
    while stack_levels(-(-cap // ipc)) > max_levels:
        cap = max(1, cap // 2)
    if item is None:
        while cap > ipc and rest - 256 - 32 * stack_levels(-(-cap // ipc)) < 40:
            cap //= 2
        room = rest - 256 - 32 * stack_levels(-(-cap // ipc))
        item = ("struct", f"{tag}i", _gen_struct(rng, f"{tag}i_", depth + 1, room, bud, caps, "list", True))
        stride = _align4(SL._lay(item, list(caps[at + 1:]), 0, True)[1])
    cap = max(1, min(cap, min(LIST_BYTES, bud.list_bytes) // stride))
    bud.list_bytes -= cap * stride
    caps[at] = cap
    return item


def random_type(rng, kind, room=None):
    """(type, caps) of a random layout of one kind."""
    room = room or {"flat": 2048, "nested": NESTED_LIMIT, "list": LIST_LIMIT}[kind]
    caps = []
    bud = _Budget(MAX_ENTRIES, MAX_RECORD - MAX_ENTRIES * 208)
    fields = _gen_struct(rng, "T", 1, room, bud, caps, kind)
    return ("struct", "t.Fuzz", fields), caps


# ---- layouts ------------------------------------------------------------------------------------------
class Layout:
    def __init__(self, name, typ, caps, origin, aimed=None):
        self.name, self.typ, self.caps, self.origin, self.aimed = name, typ, list(caps), origin, aimed
        self.fields, self.rec_len, self.pack = SL.flatten(typ, caps)
        kinds = {k for k, _, _ in self.fields}
        self.kind = "list" if LIST in kinds else "nested" if kinds & {STRUCT, VARBYTES} else "flat"
        self.peak = column_bytes(self.fields)
        self.form, self.why = verdict(self.fields, self.rec_len)
        self.accepted = self.form is not None
        self.n, self.values, self.records, self.counts = 0, [], None, []
        self.clamp = None   # (bad records, the same records with the word clamped)
        self.life = None
        self.base_off = 0

    def describe(self, i=None):
        s = f"{self.name}: {self.kind} peak {self.peak} B, record {self.rec_len} B, fields {self.fields}"
        if i is not None and i < len(self.counts):
            s += f"; record {i}: list counts {self.counts[i][0]}, []byte lengths {self.counts[i][1]}"
        return s


def _has(typ, kind):
    if typ[0] == kind:
        return True
    if typ[0] in ("ptr", "slice"):
        return _has(typ[1], kind)
    return typ[0] == "struct" and any(_has(ft, kind) for _, ft in typ[2])


def _kind_of_type(typ):
    return "list" if _has(typ, "slice") else "nested" if _has(typ, "bytes") or any(
        _has(ft, "struct") for _, ft in typ[2]) else "flat"


def _pad_to(typ, caps, target):
    """The type with raw fields in front of the top-level struct until its column peak is ``target``; None: no way."""
    fields = SL.flatten(typ, caps)[0]
    delta = target - column_bytes(fields)
    if delta < 0 or delta % 4 or (MAX_ENTRIES - len(fields)) * 8 < delta:
        return None
    pad = [(f"P{i}", U64) for i in range(delta // 8)] + ([("P", U32)] if delta % 8 else [])
    return ("struct", typ[1], pad + typ[2])


# ---- values -------------------------------------------------------------------------------------------
def _compile(t, caps, lay_kind, depth, in_item, salt):
    k = t[0]
    if k == "ptr":
        return _compile(t[1], caps, lay_kind, depth, in_item, salt)
    if k == "bool":
        return ("u", 1)
    if k == "uint":
        return ("u", t[1])
    if k == "bytearray":
        return ("ba", t[1])
    if k == "bytes":
        place = "nested" if lay_kind == "nested" else "in_item" if in_item else "list_top" if depth == 1 else "list_nested"
        salt[0] += 1
        return ("by", caps.pop(0), place, salt[0])
    if k == "struct":
        return ("st", [(name, _compile(ft, caps, lay_kind, depth + 1, in_item, salt)) for name, ft in t[2]])
    assert k == "slice"
    cap = caps.pop(0)
    item = t[1][1] if t[1][0] == "ptr" else t[1]
    if item[0] in ("bool", "uint"):
        size = 1 if item[0] == "bool" else item[1] // 8
        ik, ipc = f"raw{size}", 128 // size
    else:
        ik, ipc = ("bytes" if item[0] == "bytearray" else "struct"), 4
    salt[0] += 3
    return ("sl", cap, ipc, ik, _compile(t[1], caps, lay_kind, depth, True, salt), salt[0])


def _count_cycle(rng, cap, ipc):
    cyc = [0, 1, ipc - 1, ipc, ipc + 1, 2 * ipc, 2 * ipc + 1, cap, None, 4 * ipc + 1, None, 10 * ipc + 1, None]
    return [c if c is not None and c <= cap else rng.randint(0, cap) for c in cyc]


def _odd_levels(chunks):
    odd = 0
    while chunks > 1:
        odd += chunks & 1
        chunks = (chunks + 1) // 2
    return odd


def _draw(rng, node, i, cov, seen, full=False):
    """A value of a compiled type for record (or item) number i; ``seen``
    collects this record's list counts and []byte lengths."""
    k = node[0]
    if k == "u":
        return rng.getrandbits(node[1])
    if k == "ba":
        return rng.randbytes(node[1])
    if k == "by":
        _, cap, place, salt = node
        pick = (VAR_LENGTHS + [None, None])[(i + salt) % (len(VAR_LENGTHS) + 2)]
        L = cap if pick == "cap" else pick if pick is not None and pick <= cap else rng.randint(0, cap)
        for tag in VAR_LENGTHS:
            if L == (cap if tag == "cap" else tag):
                cov["var", place, tag] += 1
        seen[1].append(L)
        return rng.randbytes(L)
    if k == "st":
        return {name: _draw(rng, sub, i, cov, seen, full) for name, sub in node[1]}
    _, cap, ipc, ik, item, salt = node
    cyc = _count_cycle(rng, cap, ipc)
    count = cap if full else cyc[(i + salt) % len(cyc)]
    for tag, c in zip(COUNT_TAGS, [0, 1, ipc - 1, ipc, ipc + 1, 2 * ipc, 2 * ipc + 1, cap]):
        if count == c:
            cov["count", ik, tag] += 1
    if _odd_levels(-(-count // ipc)) >= 2:
        cov["odd2"] += 1
    seen[0].append(count)
    inner = ([], [])  # an item's lengths are not reported one by one
    out = [_draw(rng, item, i + j, cov, inner, full) for j in range(count)]
    seen[1].extend(sorted(set(inner[1]))[:4])
    return out


def _records(rng, lay, n, cov, full=False):
    node = _compile(lay.typ, list(lay.caps), lay.kind, 0, False, [0])
    values, counts, recs = [], [], []
    for i in range(n):
        seen = ([], [])
        v = _draw(rng, node, i, cov, seen, full)
        values.append(v)
        counts.append(seen)
        recs.append(lay.pack(v, rng.randbytes(lay.rec_len)))  # padding, slot tails and spare cells: random bytes
    rec = np.frombuffer(b"".join(recs), dtype=np.uint8).reshape(n, lay.rec_len).copy()
    return values, counts, rec


def clamp_words(fields):
    """Where a record stores a length or a count: (what, offset, capacity, list offset, stride, list capacity)."""
    out = []
    place = {f: p for f, _, p in entries_of(fields)}
    for f, (kind, off, ln) in enumerate(fields):
        if kind == VARBYTES and place[f] != "in_item":
            out.append(("var", off, ln, None, None, None))
        elif kind == LIST:
            out.append(("count", off, ln, None, None, None))
            if fields[f + 1][0] == STRUCT:
                for g in range(f + 2, f + 2 + fields[f + 1][2]):
                    if fields[g][0] == VARBYTES:
                        out.append(("item_var", fields[g][1], fields[g][2], off, fields[f + 1][1], ln))
    return out


def _draw_clamp(rng, lay, cov):
    """Three records whose lists are full, one stored word of each above its
    capacity: (bad, clamped) -- the device hashes bad as clamped, the host
    entry points refuse bad."""
    words = clamp_words(lay.fields)
    _, _, rec = _records(rng, lay, 3, Counter(), full=True)
    bad, clamped = rec.copy(), rec.copy()
    for i in range(3):
        what, off, cap, loff, stride, lcap = rng.choice(words)
        if what == "item_var":
            off += loff + 4 + rng.randrange(lcap) * stride
        over = cap + rng.choice([1, 7, 1 << 20, 0xFFFFFFFF - cap])
        bad[i, off:off + 4] = np.frombuffer(over.to_bytes(4, "little"), np.uint8)
        clamped[i, off:off + 4] = np.frombuffer(cap.to_bytes(4, "little"), np.uint8)
        cov["clamp", what] += 1
    return bad, clamped


# ---- directed layouts --------------------------------------------------------------------------------
def _rec(name, fields):
    return ("struct", name, fields)


def _directed():
    """(name, type, caps): each is there for one branch the issue names."""
    out = []
    # MK_FIELD_BYTES through the multi-block sponge at the top level of a list layout
    out.append(("bytes at the top of a list layout", _rec("t.TopBytes", [
        ("A", BA(124)), ("B", BA(128)), ("L", ("slice", U64)), ("C", BA(132)), ("D", BA(136)), ("E", BA(33)),
        ("F", BA(200)), ("G", BA(131))]), [5 * 16 + 3]))
    # every item kind at every boundary count
    small = _rec("t.Small", [("B", U16), ("A", U64)])
    var = _rec("t.Var", [("N", U64), ("D", BY), ("T", U8)])
    for nm, item, ipc, caps in [("uint8", U8, 128, []), ("uint16", U16, 64, []), ("uint32", U32, 32, []),
                                ("uint64", U64, 16, []), ("bool", BOOL, 128, []), ("bytes32", BA(32), 4, []),
                                ("bytes128", BA(128), 4, []), ("bytes132", BA(132), 4, []),
                                ("bytes136", BA(136), 4, []), ("struct", small, 4, []), ("struct var", var, 4, [133])]:
        out.append((f"items {nm}", _rec("t.Rec", [("Head", U64), ("Items", ("slice", item)), ("Tail", U16)]),
                    [10 * ipc + 3] + caps))
    # a struct item of more than one Keccak block with long byte arrays, []byte slots across the rate and a nested struct
    big = _rec("t.Big", [("N", U64), ("A", BA(128)), ("B", BA(132)), ("C", BA(136)), ("D", BY),
                         ("Sub", ("ptr", _rec("t.BigSub", [("X", U32), ("Y", BY)])))])
    out.append(("two-block struct item", _rec("t.Rec", [("Head", U64), ("Items", ("slice", ("ptr", big))), ("Tail", U16)]),
                [9, 140, 200]))
    it136 = _rec("t.I136", [(f"H{i}", BA(32)) for i in range(4)] + [("N", U64)])
    out.append(("item message of 136 B", _rec("t.Rec", [("Items", ("slice", it136)), ("T", U8)]), [9]))
    it288 = _rec("t.I288", [("V", BY)] + [(f"H{i}", BA(32 + 4 * i)) for i in range(8)])
    out.append(("item message of 288 B", _rec("t.Rec", [("Items", ("slice", it288))]), [8, 133]))
    it100 = _rec("t.I100", [("A", BA(96)), ("V", BY), ("W", BY), ("N", U32)])
    out.append(("item message of 100 B", _rec("t.Rec", [("N", U8), ("Items", ("slice", it100))]), [13, 200, 133]))
    # nested struct messages below, at and above one block, above two
    for nm, sub in [("40", [("A", U64), ("B", BA(20))]), ("136", [(f"H{i}", BA(33)) for i in range(4)] + [("N", U64)]),
                    ("168", [("V", BY)] + [(f"H{i}", BA(128 + 4 * i)) for i in range(4)] + [("N", U64)]),
                    ("288", [("V", BY)] + [(f"H{i}", BA(124 + i)) for i in range(8)])]:
        around = [("N", U64), ("T", U16)] if nm != "288" else []  # 32 + 288 B is the whole column
        out.append((f"nested message of {nm} B", _rec("t.Rec", around[:1] + [("S", ("ptr", _rec("t.Sub", sub)))] + around[1:]),
                    [c for c in [140] if any(ft == BY for _, ft in sub)]))
    # stored lengths across the rate in a nested layout and at the top of a list layout
    out.append(("[]byte slots in a nested layout", _rec("t.Rec", [
        ("A", BY), ("B", BY), ("S", _rec("t.Sub", [("C", BY), ("N", U8)])), ("D", BY)]), [200, 133, 140, 0]))
    out.append(("[]byte slots at the top of a list layout", _rec("t.Rec", [
        ("V", BY), ("L", ("slice", U16)), ("W", BY), ("X", BY)]), [200, 2 * 64 + 1, 133, 132]))
    # depth
    d4 = _rec("t.D2", [("B", U32), ("S", ("ptr", _rec("t.D3", [("C", BA(48)), ("S", _rec("t.D4", [
        ("D", BY), ("E", BA(33)), ("F", BOOL)]))])))])
    out.append(("depth 4", _rec("t.Rec", [("A", U64), ("S", ("ptr", d4)), ("Z", BY)]), [140, 64]))
    item4 = _rec("t.Item4", [("X", U64), ("Y", BY), ("Z", BA(132))])
    d3 = _rec("t.L2", [("B", U16), ("S", _rec("t.L3", [("L", ("slice", ("ptr", item4))), ("K", U8)]))])
    out.append(("list at depth 3, item struct at depth 4", _rec("t.Rec", [("A", U64), ("S", ("ptr", d3))]), [11, 133]))
    # several lists, one first and one last
    out.append(("four lists", _rec("t.Rec", [
        ("L1", ("slice", U8)), ("M", U16), ("L2", ("slice", BA(32))),
        ("S", _rec("t.Sub", [("L3", ("slice", U64)), ("Z", U8)])), ("L4", ("slice", ("ptr", small)))]),
        [2 * 128 + 1, 9, 5 * 16 + 3, 6]))
    out.append(("node stacks of 5 and 4 levels", _rec("t.Rec", [
        ("A", U8), ("L1", ("slice", U16)), ("L2", ("slice", BOOL))]), [40 * 64, 20 * 128 + 5]))
    out.append(("three lists of one chunk", _rec("t.Rec", [
        ("L1", ("slice", BOOL)), ("L2", ("slice", U32)), ("N", U64), ("L3", ("slice", BA(48)))]), [127, 32, 4]))
    return out


# ---- lives ----------------------------------------------------------------------------------------------
class Life:
    """A resident StructListTree over one layout: n0 records, then steps
    (kind, argument, first pool record, number of pool records)."""

    def __init__(self, n0):
        self.n0, self.steps, self.pool_n, self.pool = n0, [], n0, None


def _draw_life(rng, deck, script, cov):
    n0 = rng.choice([0, 1, 3, 4, 5, 8, 9, 33, 64, 65, 100])
    life = Life(n0)
    n, twin = n0, None
    for s in range(rng.randint(4, 8)):
        ok = {"update": n >= 1, "append": n + 9 <= LIFE_CAP, "erase": n >= 1, "truncate": n >= 1, "clone_diverge": n >= 1,
              "copy_from": twin is not None, "reserve": True, "audit": True, "diff": True, "branches": n >= 1}
        kind = script.pop(0) if script else None
        if kind == "erase_all" and n == 0:
            kind = None
        if kind is None or not ok.get(kind, True):
            # the deck deals every kind equally often; a card that cannot be played yet stays in it
            if not any(ok[k] for k in deck):
                deck.extend(rng.sample(LIFE_STEPS, len(LIFE_STEPS)))
            kind = next(k for k in reversed(deck) if ok[k])
            deck.reverse(), deck.remove(kind), deck.reverse()
        arg, take = None, 0
        if kind in ("update", "clone_diverge"):
            arg = TP._scattered(rng, n, 6)
            rng.shuffle(arg)  # the handle takes any order
            take = len(arg)
            if kind == "clone_diverge":
                twin = n
        elif kind == "append":
            take = rng.choice([1, 2, 3, 4, 5, 9])
            if n == 0:
                cov["append_from_empty"] += 1
            n += take
        elif kind in ("erase", "erase_all"):
            arg = list(range(n)) if kind == "erase_all" or rng.random() < 0.1 else TP._scattered(rng, n, 8)
            if len(arg) == n:
                cov["erase_all"] += 1
            rng.shuffle(arg)
            n -= len(arg)
            kind = "erase"
        elif kind == "truncate":
            arg = rng.choice([n, n - 1, rng.randint(0, n), n // 2])
            n = arg
        elif kind == "copy_from":
            n = twin
        elif kind == "diff" and twin is None:
            twin = n
        elif kind == "reserve":
            arg = rng.choice([n + 1, 2 * n + 3, n // 2, LIFE_CAP])
        elif kind == "branches":
            arg = [rng.randrange(n) for _ in range(rng.randint(1, 5))] + [0, n - 1]
        life.steps.append((kind, arg, life.pool_n, take))
        life.pool_n += take
        cov["step", kind] += 1
    return life


class LifeModel:
    """The expected state of a life: the records as a NumPy array and their
    reference roots (pool_roots: the reference root of every pool record)."""

    def __init__(self, life, pool_roots):
        self.life, self.pool_roots = life, pool_roots
        self.rec, self.roots = life.pool[:life.n0].copy(), pool_roots[:life.n0].copy()
        self.twin = None  # (records, roots) of the diverged clone

    def apply(self, step):
        """Bring the model up to date; returns what the step must observe (or None)."""
        kind, arg, first, take = step
        new, new_roots = self.life.pool[first:first + take], self.pool_roots[first:first + take]
        if kind == "update":
            self.rec[arg], self.roots[arg] = new, new_roots
        elif kind == "append":
            self.rec, self.roots = np.concatenate([self.rec, new]), np.concatenate([self.roots, new_roots])
        elif kind == "erase":
            self.rec, self.roots = np.delete(self.rec, arg, axis=0), np.delete(self.roots, arg, axis=0)
        elif kind == "truncate":
            self.rec, self.roots = self.rec[:arg].copy(), self.roots[:arg].copy()
        elif kind == "clone_diverge":
            rec, roots = self.rec.copy(), self.roots.copy()
            rec[arg], roots[arg] = new, new_roots
            self.twin = (rec, roots)
            return self.diff()
        elif kind == "copy_from":
            self.rec, self.roots = self.twin[0].copy(), self.twin[1].copy()
        elif kind == "diff":
            return self.diff()
        elif kind == "branches":
            return self.roots[arg]
        return None

    def diff(self):
        """(indices, n_self, n_other) against the twin (a fresh clone when there is none yet)."""
        if self.twin is None:
            self.twin = (self.rec.copy(), self.roots.copy())
        m = min(len(self.roots), len(self.twin[1]))
        idx = np.nonzero((self.roots[:m] != self.twin[1][:m]).any(axis=1))[0]
        return idx, len(self.roots), len(self.twin[1])

    def __len__(self):
        return len(self.rec)


# ---- tree sets ------------------------------------------------------------------------------------------
class SetPlan:
    """Trees of one TreeSet: (what, layout or item length, n0, container offset)
    and rounds of (tree, op, argument, pool first, pool count); op 'clone' has
    the set cloned, the clone changed by the round's remaining entry and the
    two diffed."""

    def __init__(self):
        self.trees, self.rounds, self.container_len, self.put = [], [], 0, None
        self.pool_n = []


def _draw_set(rng, nested, lists):
    sp = SetPlan()
    trees = [("struct", rng.choice(nested)), ("struct", rng.choice(lists)),
             rng.choice([("list", rng.choice([1, 8, 32, 48])), ("bytes", rng.choice([32, 48, 132]))])]
    if rng.random() < 0.5:
        trees.append(("struct", rng.choice(nested + lists)))
    rng.shuffle(trees)
    gaps = [rng.choice([0, 4, 8]) for _ in trees]
    off = 0
    for (what, x), g in zip(trees, gaps):
        off += g
        n0 = rng.choice([0, 1, 4, 5, 17, 33])
        sp.trees.append((what, x, n0, off))
        sp.pool_n.append(n0)
        off += 32
    sp.container_len = off + rng.choice([0, 8])
    counts = [t[2] for t in sp.trees]
    for r in range(rng.randint(3, 5)):
        ops = []
        for t in range(len(trees)):
            op = rng.choice(["update", "append", "erase", "append", None])
            if op in ("update", "erase") and counts[t] == 0:
                op = "append"
            if op == "update":
                arg = TP._scattered(rng, counts[t], 4)
                ops.append((t, op, arg, sp.pool_n[t], len(arg)))
                sp.pool_n[t] += len(arg)
            elif op == "append":
                m = rng.choice([1, 2, 5])
                ops.append((t, op, None, sp.pool_n[t], m))
                sp.pool_n[t] += m
                counts[t] += m
            elif op == "erase":
                arg = TP._scattered(rng, counts[t], 3)
                ops.append((t, op, arg, 0, 0))
                counts[t] -= len(arg)
        clone = None
        live = [t for t in range(len(trees)) if counts[t] >= 1]
        if live and rng.random() < 0.6:
            t = rng.choice(live)
            arg = TP._scattered(rng, counts[t], 3)
            clone = (t, "update", arg, sp.pool_n[t], len(arg))
            sp.pool_n[t] += len(arg)
        sp.rounds.append((ops, clone))
    return sp


# ---- the plan ---------------------------------------------------------------------------------------------
class Plan:
    def __init__(self):
        self.layouts, self.cov, self.drawn, self.dropped, self.sets = [], Counter(), 0, [], []

    @property
    def accepted(self):
        return [lay for lay in self.layouts if lay.accepted]

    @property
    def lives(self):
        return [lay for lay in self.layouts if lay.life is not None]

    def line(self):
        forms = Counter(lay.form for lay in self.accepted)
        return (f"{len(self.layouts)} layouts ({', '.join(f'{forms[f]} {f}' for f in FORMS)}, "
                f"{len(self.layouts) - len(self.accepted)} refused), {sum(lay.n for lay in self.layouts)} records, "
                f"{len(self.lives)} lives with {sum(len(lay.life.steps) for lay in self.lives)} steps, "
                f"{len(self.sets)} tree sets; {len(self.dropped)} of {self.drawn} random layouts dropped")


def _static_cov(lay, cov):
    fields = lay.fields
    ents = entries_of(fields)
    cov["form", lay.form] += 1
    cov["peak", lay.kind, lay.peak] += 1
    nlists = sum(k == LIST for k, _, _ in fields)
    if lay.kind == "nested" and struct_depth(fields) == 4:
        cov["nested depth 4"] += 1
    if nlists >= 3:
        cov["three lists"] += 1
    if fields[0][0] == LIST:
        cov["list first"] += 1
    if any(fields[f][0] == LIST and f + SL._span(fields, f) == len(fields) and d == 1 for f, d, _ in ents):
        cov["list last"] += 1
    for f, d, place in ents:
        kind, _, ln = fields[f]
        if kind == LIST:
            cov["levels", stack_levels(list_chunks(fields, f))] += 1
            if d == 3 and fields[f + 1][0] == STRUCT:
                cov["list at depth 3, item struct at depth 4"] += 1
        if kind == BYTES and lay.kind == "list":
            where = {"top": "list_top", "item": "item", "in_item": "in_item"}.get(place)
            cov["bytes", where, ln] += 1
            if where == "list_top" and ln % 2:
                cov["bytes", where, "odd"] += 1
            if where == "list_top" and ln >= 200:
                cov["bytes", where, ">=200"] += 1
        if kind == STRUCT:
            m = msg_len(fields, f + 1, f + 1 + ln)
            where = "item" if place == "item" else "nested" if lay.kind == "nested" else None
            for tag, hit in [("<136", m < 136), ("136", m == 136), (">136", m > 136), (">272", m > 272)]:
                if hit and where:
                    cov["msg", where, tag] += 1


def _n_for(lay, i):
    fit = [n for n in RECORD_COUNTS if n * lay.rec_len <= RECORDS_BYTES] or [1]
    return fit[-1] if RECORD_COUNTS[i % len(RECORD_COUNTS)] > fit[-1] else RECORD_COUNTS[i % len(RECORD_COUNTS)]


@lru_cache(maxsize=None)
def plan():
    p = Plan()
    rng = random.Random(SEED + 1)
    cands = [(name, typ, caps, "directed", None) for name, typ, caps in _directed()]
    # column peaks on and 4 B above each switch and limit
    for kind, targets in [("nested", [160, 164, 320, 324]), ("list", [320, 324, 640, 644])]:
        for target in targets:
            made = 0
            while made < PEAK_LAYOUTS:
                typ, caps = random_type(rng, kind, room=target)
                padded = _pad_to(typ, caps, target) if _kind_of_type(typ) == kind else None
                if padded is not None:
                    cands.append((f"{kind} peak {target} #{made}", padded, caps, "peak", target))
                    made += 1
    for kind, count in RANDOM_LAYOUTS.items():
        for i in range(count * SCALE):
            typ, caps = random_type(rng, kind.rstrip("128"), LIST_SWITCH if kind == "list128" else None)
            cands.append((f"random {kind} #{i}", typ, caps, "random", None))
    for i, (name, typ, caps, origin, aimed) in enumerate(cands):
        lay = Layout(name, typ, caps, origin, aimed)
        if origin == "random":
            p.drawn += 1
            if not lay.accepted or lay.rec_len > MAX_RECORD:
                p.dropped.append((name, lay.why or f"record of {lay.rec_len} B"))
                continue
        assert lay.rec_len <= MAX_RECORD, lay.describe()
        lay.base_off = 4 if len(p.layouts) % 2 else 0
        p.layouts.append(lay)
    # records, clamp variants and lives: streams of their own, so that a change of one leaves the others alone
    vr, cr, lr = random.Random(SEED + 2), random.Random(SEED + 3), random.Random(SEED + 4)
    deck, nlife = [], 0
    for i, lay in enumerate(p.accepted):
        _static_cov(lay, p.cov)
        lay.n = _n_for(lay, i)
        lay.values, lay.counts, lay.records = _records(vr, lay, lay.n, p.cov)
        if clamp_words(lay.fields) and i % 10 == 3:
            lay.clamp = _draw_clamp(cr, lay, p.cov)
        if lay.kind != "flat" and i % 4 == 1 and lay.rec_len <= 4096:
            script = [["append"], ["update", "erase_all", "append"], [], []][nlife % 4]
            lay.life = _draw_life(lr, deck, list(script), p.cov)
            lay.life.pool = _records(lr, lay, lay.life.pool_n, Counter())[2]
            nlife += 1
    sr = random.Random(SEED + 5)
    small = [lay for lay in p.accepted if lay.rec_len <= 2048]
    nested, lists = [lay for lay in small if lay.kind == "nested"], [lay for lay in small if lay.kind == "list"]
    p.sets = [_draw_set(sr, nested, lists) for _ in range(TREE_SETS)]
    return p


def set_pool(sp, t, salt):
    """The records (or items) tree t of a set draws from, in the order its ops take them."""
    what, x, _, _ = sp.trees[t]
    rng = random.Random(SEED + 6000 + salt)
    if what == "struct":
        return _records(rng, x, sp.pool_n[t], Counter())[2]
    return np.frombuffer(rng.randbytes(max(sp.pool_n[t], 1) * x), np.uint8).reshape(-1, x)[:sp.pool_n[t]].copy()
