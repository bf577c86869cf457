"""The packed SR compiler's word table (evogp_amd/csrc/sr_tc.hip tc_table_entry) restated twice in Python.

`entry(code, recip, H)` is the table as the engine builds it: one 64-bit entry per class code.  `by_selects(code, recip, H)` derives the
same fields the way the compiler's select chains do (compile_pack_arith without the table, compile_tree_arith): from the lane's
predicates -- is it a binary node, a leaf, folded in the first round, the root; its operator; its operands' kinds -- through id / fn_id,
division_in_place, no_prefetch_delta, kept, uses-a-variable and the stack delta.  tests/test_tc_word_table.py holds the two against each
other and against the engine's own table for every class code.  H: {handler name: id} of evogp_amd/lib/tc_handlers.json.

Class code: opx | pair << 2 | root << 6 for a binary node (opx: 0 + 1 - 2 * 3 /; pair = 3 kl + kr, operand kinds 0 V, 1 C, 2 on the stack;
9: folded in the first round); OTHER + kind for the rest (0 V, 1 C, 3 / 5 a node whose tree is handed on); NOFN + 0 / 1 / 2 for the unary "no
function" (pushes 0 / folded to the constant 0 in the first round / the generic stub).
Entry: ids = id | twin << 8 | in-place id << 16 | in-place twin << 24; bits = room | (delta + 1) << 24 | (kept and uses a variable) << 26 |
leaf << 27 | kept << 31."""
ROOT, ABSORBED, OTHER, NOFN, CODES = 64, 9 << 2, 11 << 2, 13 << 2, 128
NO_ROOM, ROOM_MASK, USES_KEPT, LEAF, KEPT, DELTA_SHIFT = 1 << 22, 0xFFFFFF, 1 << 26, 1 << 27, 1 << 31, 24
FORMS = ["ss", "sv", "vs", "sc", "cs", "vv", "vc", "cv"]
OPS = ["add", "sub", "mul", "div"]
FORM_OF_PAIR = [5, 6, 2, 7, 0, 4, 1, 3, 0]   # 3 kl + kr -> form; (C, C) has none: folded


def handler_ids(table):
    """{name: id} from the "handlers" object of one build in tc_handlers.json"""
    return {name.lower(): v["id"] for name, v in table.items()}


def pack(ident, twin, ip, iptwin, room, delta, kept, uses, leaf):
    ids = ident | (ident + twin) << 8 | ip << 16 | (ip + iptwin) << 24
    bits = room | (delta + 1) << DELTA_SHIFT | (USES_KEPT if kept and uses else 0) | (LEAF if leaf else 0) | (KEPT if kept else 0)
    return ids, bits


def entry(code, recip, H):
    root, c = bool(code & ROOT), code & 63
    opx, pair = c & 3, c >> 2
    push_twin, ip_twin = H["push_c_np"] - H["push_c"], H["divip_ss_np"] - H["divip_ss"]
    ident = twin = delta = 0
    ip, kept, uses, leaf, room = -1, False, False, False, NO_ROOM
    if pair <= 8:
        kl, kr = divmod(pair, 3)
        kept, delta = True, (kl != 2) + (kr != 2) - 1
        if (kl, kr) == (1, 1):
            ident, twin = H["push_c"], push_twin
        else:
            form = FORM_OF_PAIR[pair]
            uses = kl == 0 or kr == 0
            if recip and opx == 3 and kr == 0:
                ident, twin = H["divr_sv"] + (form * 3 >> 3), H["divr_sv_np"] - H["divr_sv"]
            else:
                ident, twin = opx * 8 + form, H["add_ss_np"] if opx < 3 else 0
                if opx == 3 and form in (0, 3, 4):
                    ip, room = H["divip_ss"] + (0, None, None, 1, 2)[form], 1 if form == 0 else 0
    elif c in (ABSORBED, NOFN + 1):
        ident, twin, kept, delta = H["push_c"], push_twin, root, int(root)
    elif c in (OTHER, OTHER + 1):
        ident, leaf, kept, uses, delta = int(c == OTHER), True, root, c == OTHER, int(root)
    elif c == NOFN:
        ident, twin, kept, delta = H["push_c"], push_twin, True, 1
    elif c == NOFN + 2:
        ident, kept = H["gun_s"], True
    if ip < 0:
        ip = ident
    return pack(ident, twin, ip, twin if room == NO_ROOM else ip_twin, room, delta, kept, uses, leaf)


def predicates(code):
    """the lane of a class code as the select chains see it, or None for a code no lane can have"""
    root, c = bool(code & ROOT), code & 63
    opx, pair = c & 3, c >> 2
    lane = dict(root=root, opx=opx, B=False, V=False, C=False, U=False, absorbed=False, stub=False, kl=1, kr=1)
    if pair <= 8:
        lane.update(B=True, kl=pair // 3, kr=pair % 3)
    elif c == ABSORBED:
        lane.update(B=True, absorbed=True)
    elif c in (OTHER, OTHER + 1):
        lane.update(V=c == OTHER, C=c == OTHER + 1)
    elif c in (OTHER + 3, OTHER + 5):
        pass
    elif c in (NOFN, NOFN + 1, NOFN + 2):
        lane.update(U=True, absorbed=c == NOFN + 1, stub=c == NOFN + 2, kl=(0, 1, 2)[c - NOFN])
    else:
        return None
    return lane


def by_selects(code, recip, H, twins_on=True):
    """-> {(next word reads a variable, room on the stack): handler id} and (kept, uses a variable, delta, is a leaf) of the lane, through
    the compiler's own chain: id, division_in_place, no_prefetch_delta.  The leaf's id is relative to TcCompileParams::leaf_id."""
    p = predicates(code)
    if p is None:
        return None
    B, V, U, root, opx, kl, kr = p["B"], p["V"], p["U"], p["root"], p["opx"], p["kl"], p["kr"]
    leafnode = V or p["C"]
    absorbed = p["absorbed"]
    cc = B and not absorbed and kl == 1 and kr == 1
    stub = U and not absorbed and kl == 2
    pushc = absorbed or cc or (U and not stub)
    kept = ((B or U) and (not absorbed or root)) or (root and leafnode)
    divr = B and opx == 3 and kr == 0 and bool(recip)
    form = FORM_OF_PAIR[min(kl * 3 + kr, 8)]
    # by NAME from here on: the table's arithmetic on ids (8 opx + form, + the twin's distance) has to land on these handlers
    fn = f"divr_{FORMS[form]}" if divr else f"{OPS[opx]}_{FORMS[form]}"
    name = "push_c" if pushc else fn if B else "gun_s" if stub else None   # (None: a leaf, TcCompileParams::leaf_id + V)
    delta = int(kept) if absorbed else (kl != 2) + (kr != 2) - 1 if B else (0 if stub else 1) if U else int(root and leafnode)
    uses = not pushc and not U and ((B and (kl == 0 or kr == 0)) or (not B and V))
    divown = B and not pushc and not divr and opx == 3
    can_ip = divown and form in (0, 3, 4)
    out = {}
    for nxt in (True, False):
        for room in (True, False):
            name2 = f"divip_{FORMS[form]}" if can_ip and room else name
            twin = (B and not pushc and not divr and opx < 3) or pushc or (can_ip and room) or (divr and not pushc)   # no_prefetch_delta's four cases
            if twins_on and not nxt and twin:
                name2 += "_np"
            out[nxt, room] = int(V) if name2 is None else H[name2]
    return out, (kept, uses, delta, leafnode), (1 if form == 0 else 0) if can_ip else None


def from_entry(ids, bits):
    """the same view of an entry: what compile_pack_arith makes of it"""
    out = {}
    room = bits & ROOM_MASK
    for nxt in (True, False):
        for has_room in (True, False):
            w = ids if nxt else ids >> 8
            out[nxt, has_room] = (w >> 16 if has_room and room != NO_ROOM else w) & 0xFF
    kept = bool(bits & KEPT)
    return out, (kept, bool(bits & USES_KEPT), ((bits >> DELTA_SHIFT) & 3) - 1, bool(bits & LEAF)), None if room == NO_ROOM else room
