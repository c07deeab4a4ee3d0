#!/usr/bin/env python3
"""Generates phyly_amd/csrc/plk_fused4_v4_asm.h: the CDNA4 assembly text of the k = 4 pair-table interpreter with TWO
sites per lane (k_ll_fused4_v4, plk_fused4_v4.h).

Why a generator: every handler exists once per stack slot and every vector instruction twice (site A, site B,
interleaved so that the two independent dependency chains alternate in the issue stream); written as C macros that is
~700 lines of hand-numbered registers.  The register map, the handler numbering and the op-word format are defined
here once and the header is emitted from them.  Run `python tools/gen_fused4_v4.py` after changing this file; the header
is committed, the build does not depend on Python.

Op format (built by plk_fused_v4_words in plk_program.h from the pair-table program): 64 bits per op, blocks of 8 ops
(7 ops of the program and one REFILL op, see below),
  lo dword  handler index * 512 (byte offset of the handler in the table; the table is 32 KB aligned)
  hi dword  observation ops: bits 31:16 = LDS offset / 32 of the table the NEXT observation op reads, bits 15:0 = LDS
            offset / 64 of the staged code row of the observation op AFTER the next (both relative to LDS address 0)
Handler indices: 0 TIP_SET, 1 TIP_MUL, 2 MATVEC, 3 TIP_MUL without wait, 4 MATVEC + TIP_MUL, 6 SCALE, 7 END,
8 + d PUSH slot d, 12 + d TIP_SET + POPMUL slot d, 16 + d POPMUL slot d, 20 + d TIP_SET + PUSH slot d,
24 + d MATVEC + PUSH slot d, 28 + d MATVEC + POPMUL slot d (d < 4), 32 REFILL_A, 33 REFILL_B.

Dispatch is THREADED: there is no interpreter loop.  Two op blocks (16 ops, 32 dwords) sit in s[68:99] as a ring that
M0 indexes; every handler ends in NEXT = { s_movrels_b64 op, ring[M0]; M0 += 2; target = table | op.lo; s_setpc target },
one taken jump per op instead of two (call + return).  The last op of a block is a REFILL: executed when its block has
been consumed, it waits for the other block (requested one block earlier), requests the block after that into its own
half of the ring (REFILL_B also wraps M0 to 0) and goes on.  The program buffer therefore ends with two spare blocks.

Registers (all named in the clobber list of the asm statement):
  v[24:31] xA  v[32:39] xB   vectors under construction (site A = lane's first site, site B = HALF sites further)
  v[40:47] tA  v[48:55] tB   product accumulators
  v[56:63] pA  v[64:71] pB   prefetched tip / pair-table value of the next observation op
  v72 v73 value addresses   v74 v75 code bytes of the next observation op   v76 code address   v77 LDS address of the
  lane's byte in row 0 (site A; site B at +HALF)   v78 v79 scale exponents   v80 v81 temporaries
  v[82:145] stack: slot d = A v[82+16d : 89+16d], B v[90+16d : 97+16d]
  s[36:67] current matrix (transposed)   s[68:99] ring of two op blocks, indexed by M0 (dwords)
  s[20:21] program pointer (next block to request)   s[22:23] the op being executed (s23 = its fields)
  s[24:25] jump target (s25 = high half of the table address, constant)   s26 low half of the table address
  s27 = -1022   s28 s29 temporaries   s[30:31] matrix stream pointer

Second emission mode, STREAMED codes (k_ll_fused4_v4s, plk_fused4_v4s.h -> plk_fused4_v4s_asm.h): the codes of the
observation ops do not sit in LDS rows, they arrive packed four to a dword from a stream in global memory that holds a
128-site unit's bytes in program order (plk_stream_dword in plk_program.h).  What differs from the text above:
  hi dword  observation ops: bits 31:16 = LDS offset / 32 of the table the NEXT observation op reads (the category's base
            included), bits 4:0 = bit offset (0 / 8 / 16 / 24) of that observation's code in the current dword
  v[74:75]  the current dword of site A | site B   v76 lane * 8 (offset of the lane's dword pair in a chunk)
  v[146:147] v[148:149]  the two chunks in flight   s[34:35] stream pointer (next chunk to request)   v77 unused
  handlers 34 + k (k < 2) ADVANCE_k: wait for the older of the two chunks in flight, make it the current dword and
  request the chunk after next into its register pair.  The op stream holds an ADVANCE before the observation op that
  extracts the first byte of a new dword, kinds alternating from 0.
  FOLDED handlers (plk_v4s_fold_ops in plk_program.h retargets ops of the checked stream at them; each is the text of
  the two handlers it stands for under one dispatch, so what a site computes does not change):
  36 + 2 j + k   observation handler OBS_HANDLERS[j] with ADVANCE_k between its arithmetic and its extraction
  60 + d         MATVEC + POPMUL slot d, then SCALE
  Two prologues over one handler table: PLK_V4S_PROLOGUE requests the unit's first three chunks itself and waits for the
  first; PLK_V4S_PROLOGUE_HELD copies them from three 64-bit operands that the kernel loaded once per unit.
  Scalar operands: %[rec], the category's record (PlkV4SRecord in plk_program.h: op stream, matrix stream, first_y, first_y1,
  first_b1 at bytes 0 .. 27, the four root weights at 32 .. 63), and %[strm], the unit's code stream.  The prologue loads the
  record's first half and moves its fields to where the handlers expect them; s[32:33] keeps the record's address and the
  epilogue loads the weights from it into s[20:27], which are dead by then.

Third emission mode, PAIR PRODUCTS (k_ll_fused4_v4s<768, true, true>, plk_fused4_v4s.h -> plk_fused4_v4p_asm.h): the streamed form for
programs that need at most 3 stack slots.  The registers of stack slot 3 are a second look-up buffer: the row of
observation n lands in buffer n & 1 (buffer 0 = v[56:71], buffer 1 = v[130:145]), an observation handler consumes its own
buffer and requests observation n + 2 into it (the chain is two ahead; the prologue starts it with observations 0 and 1),
and a PAIR handler forms x = P[n] * P[n + 1] from both buffers with one multiply per state and site -- what TIP_SET n,
TIP_MUL n + 1 and TIP_SET + PUSH d, TIP_SET + POPMUL d compute with eight moves more -- and requests n + 2 and n + 3.
What differs from the streamed text above:
  hi dword  observation ops: the fields name the observation TWO after the op's (clamped to the last one)
            PAIR ops: bits 1:0 byte of observation n + 2 in its dword, bits 4:3 byte of observation n + 3, bits 17:5 and
            bits 30:18 LDS offset / 32 of their tables (bits 2 and 31 are zero)
  The table keeps its 64 slots of 512 bytes (the compiler's branches across the statement stay within their 16-bit reach).
  Indices 2, 6, 7, 8 + d, 16 + d, 24 + d, 28 + d, 32, 33, 34 + k and 60 + d as above with d < 3: no handler touches slot 3.
  The extraction that needs a new dword is the one of an observation with an index that is a multiple of 4: two ahead, it
  falls into the handler of an even observation, the first of a PAIR of an even one or the second of a PAIR of an odd one,
  so handlers with an ADVANCE inside exist for those parities only.
  PAIR_OBS_HANDLERS[j] on buffer 0    its index of the streamed table (0, 1, 3, 4, 12 + d, 20 + d)
  PAIR_OBS_HANDLERS[j] on buffer 1    PAIR_OBS_ODD[j] (5, 11, 15, 19, 23, 27, 31, none, 59, 63)
  36 + 2 jj + k   observation handler PAIR_OBS_FOLDED[jj] on buffer 0 with ADVANCE_k before its extraction (all but TIP_SET
                  alone and TIP_MUL without wait, which binary trees do not produce: their ADVANCE keeps its dispatch)
  TIP_SET + PUSH slot 0 exists on buffer 0 without ADVANCE only: a look-up goes to slot 0 when the stack is empty and no
  vector is under construction, which in every tree tried is the program's first observation (tests/pairmulcheck_main.cpp
  finds no other); a program that had it on buffer 1 gets no pair-product stream and runs the folded one.
  52, 53 + k      PAIR of an even observation: no ADVANCE, ADVANCE_k before the first extraction
  55, 56 + k      PAIR of an odd observation: no ADVANCE, ADVANCE_k between the two extractions
"""
import os

HS = 512                      # bytes per handler slot
XA, XB, TA, TB, PA, PB = 24, 32, 40, 48, 56, 64
STACK0 = 82


def pair(r):
    return "v[%d:%d]" % (r, r + 1)


def slot_regs(d, site):
    base = STACK0 + 16 * d + 8 * site
    return [base + 2 * i for i in range(4)]


def matvec(dst_a=None, dst_b=None):
    """x = M x for both sites, rows interleaved A/B; dst_*: registers of the result (default in place)"""
    out = ["s_waitcnt lgkmcnt(0)"]
    for col in range(4):
        for row in range(4):
            s = 36 + 8 * col + 2 * row
            for (x, t, dst) in ((XA, TA, dst_a), (XB, TB, dst_b)):
                xin = pair(x + 2 * col)
                acc = pair(t + 2 * row)
                if col == 0:
                    out.append("v_mul_f64 %s, s[%d:%d], %s" % (acc, s, s + 1, xin))
                elif col < 3:
                    out.append("v_fma_f64 %s, s[%d:%d], %s, %s" % (acc, s, s + 1, xin, acc))
                else:
                    d = pair((dst[row]) if dst else x + 2 * row)
                    out.append("v_fma_f64 %s, s[%d:%d], %s, %s" % (d, s, s + 1, xin, acc))
    out += ["s_add_u32 s30, s30, 0x80", "s_addc_u32 s31, s31, 0",
            "s_load_dwordx16 s[36:51], s[30:31], 0x0", "s_load_dwordx16 s[52:67], s[30:31], 0x40"]
    return out


def tipmul(buf=PA):
    """buf: first register of the look-up buffer (site A; site B 8 registers further)"""
    out = []
    for i in range(4):
        out.append("v_mul_f64 %s, %s, %s" % (pair(XA + 2 * i), pair(XA + 2 * i), pair(buf + 2 * i)))
        out.append("v_mul_f64 %s, %s, %s" % (pair(XB + 2 * i), pair(XB + 2 * i), pair(buf + 8 + 2 * i)))
    return out


def tipset(buf=PA):
    out = []
    for i in range(4):
        out.append("v_mov_b64 %s, %s" % (pair(XA + 2 * i), pair(buf + 2 * i)))
        out.append("v_mov_b64 %s, %s" % (pair(XB + 2 * i), pair(buf + 8 + 2 * i)))
    return out


def pairmul(first, second):
    """x = first buffer o second buffer: TIP_SET of the first and TIP_MUL of the second without the copy"""
    out = []
    for i in range(4):
        out.append("v_mul_f64 %s, %s, %s" % (pair(XA + 2 * i), pair(first + 2 * i), pair(second + 2 * i)))
        out.append("v_mul_f64 %s, %s, %s" % (pair(XB + 2 * i), pair(first + 8 + 2 * i), pair(second + 8 + 2 * i)))
    return out


def tipnext():
    return ["s_lshr_b32 s28, s23, 16", "s_and_b32 s29, s23, 0xffff",
            "v_add_lshl_u32 v72, v74, s28, 5", "v_add_lshl_u32 v73, v75, s28, 5",
            "ds_read_b128 v[56:59], v72", "ds_read_b128 v[60:63], v72 offset:16",
            "ds_read_b128 v[64:67], v73", "ds_read_b128 v[68:71], v73 offset:16",
            "v_lshl_add_u32 v76, s29, 6, v77",
            "ds_read_u8 v74, v76", "@HALF ds_read_u8 v75, v76"]


def lookup(buf, bits, table):
    """request the rows of the codes at bit offset `bits` of the current dwords from table `table` into buffer buf"""
    return ["v_bfe_u32 v72, v74, %s, 8" % bits, "v_bfe_u32 v73, v75, %s, 8" % bits,
            "v_add_lshl_u32 v72, v72, %s, 5" % table, "v_add_lshl_u32 v73, v73, %s, 5" % table,
            "ds_read_b128 v[%d:%d], v72" % (buf, buf + 3), "ds_read_b128 v[%d:%d], v72 offset:16" % (buf + 4, buf + 7),
            "ds_read_b128 v[%d:%d], v73" % (buf + 8, buf + 11), "ds_read_b128 v[%d:%d], v73 offset:16" % (buf + 12, buf + 15)]


def tipnext_s(buf=PA):
    # v_bfe_u32 reads bits 4:0 of its offset operand only: the op's field dword serves as it is
    return ["s_lshr_b32 s28, s23, 16"] + lookup(buf, "s23", "s28")


def pairnext(which, buf):
    """the two requests of a PAIR op: field layout in the module text"""
    if which == 0:
        return ["s_lshl_b32 s28, s23, 3", "s_bfe_u32 s29, s23, 0xd0005"] + lookup(buf, "s28", "s29")
    return ["s_and_b32 s28, s23, 0x18", "s_lshr_b32 s29, s23, 18"] + lookup(buf, "s28", "s29")


RING = (146, 148)             # streamed mode: register pairs of the two chunks in flight
CHUNK_BYTES = 512             # one wave-wide dwordx2 load


def advance(k):
    return ["s_waitcnt vmcnt(1)", "v_mov_b64 v[74:75], %s" % pair(RING[k]),
            "global_load_dwordx2 %s, v76, s[34:35]" % pair(RING[k]),
            "s_add_u32 s34, s34, 0x%x" % CHUNK_BYTES, "s_addc_u32 s35, s35, 0"]


def push(d):
    out = []
    for i in range(4):
        out.append("v_mov_b64 %s, %s" % (pair(slot_regs(d, 0)[i]), pair(XA + 2 * i)))
        out.append("v_mov_b64 %s, %s" % (pair(slot_regs(d, 1)[i]), pair(XB + 2 * i)))
    return out


def popmul(d):
    out = []
    for i in range(4):
        out.append("v_mul_f64 %s, %s, %s" % (pair(XA + 2 * i), pair(XA + 2 * i), pair(slot_regs(d, 0)[i])))
        out.append("v_mul_f64 %s, %s, %s" % (pair(XB + 2 * i), pair(XB + 2 * i), pair(slot_regs(d, 1)[i])))
    return out


def setpop(d, buf=PA):
    """x = prefetched value o slot d (TIP_SET followed by POPMUL: no copy of the value)"""
    out = []
    for i in range(4):
        out.append("v_mul_f64 %s, %s, %s" % (pair(XA + 2 * i), pair(buf + 2 * i), pair(slot_regs(d, 0)[i])))
        out.append("v_mul_f64 %s, %s, %s" % (pair(XB + 2 * i), pair(buf + 8 + 2 * i), pair(slot_regs(d, 1)[i])))
    return out


def setpush(d, buf=PA):
    """slot d = prefetched value (TIP_SET followed by PUSH: the vector under construction is dead after a PUSH)"""
    out = []
    for i in range(4):
        out.append("v_mov_b64 %s, %s" % (pair(slot_regs(d, 0)[i]), pair(buf + 2 * i)))
        out.append("v_mov_b64 %s, %s" % (pair(slot_regs(d, 1)[i]), pair(buf + 8 + 2 * i)))
    return out


def scale():
    out = []
    for (x, tmp, esc) in ((XA, 80, 78), (XB, 81, 79)):
        out += ["v_max_u32 v%d, v%d, v%d" % (tmp, x + 1, x + 3), "v_max3_u32 v%d, v%d, v%d, v%d" % (tmp, x + 5, x + 7, tmp),
                "v_lshrrev_b32 v%d, 20, v%d" % (tmp, tmp), "v_sub_u32 v72, 0x3fe, v%d" % tmp]
        out += ["v_ldexp_f64 %s, %s, v72" % (pair(x + 2 * i), pair(x + 2 * i)) for i in range(4)]
        out.append("v_add3_u32 v%d, v%d, v%d, s27" % (esc, esc, tmp))
    return out


# NEXT: fetch the op the ring index points at and jump to its handler (s_movrels reads M0: M0 is written after it, never
# within one instruction before it)
RET = ["s_movrels_b64 s[22:23], s[68:69]", "s_addk_i32 m0, 0x2", "s_or_b32 s24, s26, s22", "s_setpc_b64 s[24:25]"]
NSLOTS = 64
REFILL_A, REFILL_B = 32, 33
ADVANCE0 = 34


OBS_HANDLERS = (0, 1, 3, 4, 12, 13, 14, 15, 20, 21, 22, 23)     # in the order of their folded variants
FOLD_ADV0 = 36                # 36 + 2 j + k: OBS_HANDLERS[j] with ADVANCE_k before its extraction
FOLD_SCALE0 = 60              # 60 + d: MATVEC + POPMUL slot d, then SCALE


def obs_handlers(tipnext, buf=PA, slots=4):
    """the observation handlers (OBS_HANDLERS) without their dispatch; tipnext: the prefetch of the next observation; buf:
    the look-up buffer they consume; slots: stack slots they exist for"""
    h = {}
    h[0] = ["s_waitcnt lgkmcnt(0)"] + tipset(buf) + tipnext()
    h[1] = ["s_waitcnt lgkmcnt(0)"] + tipmul(buf) + tipnext()
    h[3] = tipmul(buf) + tipnext()
    h[4] = matvec() + tipmul(buf) + tipnext()
    for d in range(slots):
        h[12 + d] = ["s_waitcnt lgkmcnt(0)"] + setpop(d, buf) + tipnext()
        h[20 + d] = ["s_waitcnt lgkmcnt(0)"] + setpush(d, buf) + tipnext()
    assert tuple(sorted(h)) == (OBS_HANDLERS if slots == 4 else PAIR_OBS_HANDLERS)
    return h


# ---- pair products: two look-up buffers, the chain two ahead ----
BUF = (PA, STACK0 + 48)       # buffer 1 = the registers of stack slot 3
PAIR_SLOTS = 3
PAIR_OBS_HANDLERS = (0, 1, 3, 4, 12, 13, 14, 20, 21, 22)       # on buffer 0: the streamed table's indices
PAIR_OBS_ODD = (5, 11, 15, 19, 23, 27, 31, None, 59, 63)       # the same handlers on buffer 1
PAIR_OBS_FOLDED = (1, 4, 12, 13, 14, 21, 22)                   # 36 + 2 jj + k: on buffer 0 with ADVANCE_k inside
PAIR_FOLD0 = 36
PAIR_EVEN0, PAIR_ODD0 = 52, 55


def pair_handlers():
    h = {2: matvec() + RET, 6: scale() + RET, 7: ["s_branch .Ldone_%="]}
    for d in range(PAIR_SLOTS):
        h[8 + d] = push(d) + RET
        h[16 + d] = popmul(d) + RET
        h[24 + d] = matvec(slot_regs(d, 0), slot_regs(d, 1)) + RET
        h[28 + d] = matvec() + popmul(d) + RET
        h[FOLD_SCALE0 + d] = matvec() + popmul(d) + scale() + RET
    full = handlers(True)
    for idx in (REFILL_A, REFILL_B, ADVANCE0, ADVANCE0 + 1):
        h[idx] = full[idx]
    for p in range(2):
        obs = obs_handlers(lambda: tipnext_s(BUF[p]), BUF[p], PAIR_SLOTS)
        for j, idx in enumerate(PAIR_OBS_HANDLERS):
            if (PAIR_OBS_HANDLERS, PAIR_OBS_ODD)[p][j] is not None:
                h[(PAIR_OBS_HANDLERS, PAIR_OBS_ODD)[p][j]] = obs[idx] + RET
    for k in range(2):
        obs = obs_handlers(lambda: advance(k) + tipnext_s(BUF[0]), BUF[0], PAIR_SLOTS)
        for jj, idx in enumerate(PAIR_OBS_FOLDED):
            h[PAIR_FOLD0 + 2 * jj + k] = obs[idx] + RET

    def pair_handler(p, before, between):
        return (["s_waitcnt lgkmcnt(0)"] + pairmul(BUF[p], BUF[1 - p]) + before + pairnext(0, BUF[p]) + between +
                pairnext(1, BUF[1 - p]) + RET)
    h[PAIR_EVEN0] = pair_handler(0, [], [])
    h[PAIR_ODD0] = pair_handler(1, [], [])
    for k in range(2):
        h[PAIR_EVEN0 + 1 + k] = pair_handler(0, advance(k), [])
        h[PAIR_ODD0 + 1 + k] = pair_handler(1, [], advance(k))
    assert sorted(set(range(NSLOTS)) - set(h)) == [50, 51, 58]       # 22 + 19 + 14 + 6 handlers
    return h


def handlers(streamed=False):
    tipnext = tipnext_s if streamed else globals()["tipnext"]
    h = {idx: body + RET for idx, body in obs_handlers(tipnext).items()}
    h[2] = matvec() + RET
    h[6] = scale() + RET
    h[7] = ["s_branch .Ldone_%="]
    for d in range(4):
        h[8 + d] = push(d) + RET
        h[16 + d] = popmul(d) + RET
        h[24 + d] = matvec(slot_regs(d, 0), slot_regs(d, 1)) + RET
        h[28 + d] = matvec() + popmul(d) + RET
    adv = ["s_add_u32 s20, s20, 0x40", "s_addc_u32 s21, s21, 0"]
    h[REFILL_A] = ["s_waitcnt lgkmcnt(0)", "s_load_dwordx16 s[68:83], s[20:21], 0x0"] + adv + RET
    h[REFILL_B] = ["s_mov_b32 m0, 0", "s_waitcnt lgkmcnt(0)", "s_load_dwordx16 s[84:99], s[20:21], 0x0"] + adv + RET
    if streamed:
        for k in range(2):
            h[ADVANCE0 + k] = advance(k) + RET
            # folded: the handler's own arithmetic, then ADVANCE_k, then its extraction, which reads the new current dword
            for j, (idx, body) in enumerate(sorted(obs_handlers(lambda: advance(k) + tipnext_s()).items())):
                h[FOLD_ADV0 + 2 * j + k] = body + RET
        for d in range(4):
            h[FOLD_SCALE0 + d] = matvec() + popmul(d) + scale() + RET
    return h


def emit(streamed=False, held=False, pairs=False):
    """-> (prologue up to the dispatch of the first op, handler table and epilogue)"""
    L = []           # (text, is_label)

    def ins(lines):
        for t in lines:
            L.append(t)

    # ---- prologue ----
    pro = []
    if streamed:
        # what is per category and per launch comes from the category's record in device memory (PlkV4SRecord, plk_program.h):
        # one scalar load, requested first so that the vector moves below run while it travels, into registers of the first
        # matrix, which is requested after the record's fields have been moved out.  The record's address stays in s[32:33]
        # for the root weights (epilogue).  The statement's scalar operands are the record and the stream pointer and nothing
        # else: what the kernel's loop keeps in scalar registers stays there.
        pro += ["s_load_dwordx8 s[36:43], %[rec], 0x0", "s_mov_b64 s[32:33], %[rec]"]
    for i in range(4):
        pro += ["v_mov_b32 v%d, 0" % (XA + 2 * i), "v_mov_b32 v%d, 0x3ff00000" % (XA + 2 * i + 1),
                "v_mov_b32 v%d, 0" % (XB + 2 * i), "v_mov_b32 v%d, 0x3ff00000" % (XB + 2 * i + 1)]
    if held:
        # the first three chunks are operands: the kernel requested them once per unit (the compiler waits for them before the
        # statement, which costs time in the unit's first category only).  Vector memory operations of the kernel may still be
        # in flight here and none of the statement's own is: ADVANCE's s_waitcnt vmcnt(1) assumes two loads of its own in
        # flight, and fewer of them, or older operations in front of them (the counter retires in order), only make it wait
        # for less or for more than the chunk it needs, never for too little
        pro += ["v_mov_b32 v76, %[voff]", "s_mov_b64 s[34:35], %[strm]",
                "v_mov_b64 v[74:75], %[c0]", "v_mov_b64 %s, %%[c1]" % pair(RING[0]), "v_mov_b64 %s, %%[c2]" % pair(RING[1]),
                "s_add_u32 s34, s34, 0x%x" % (3 * CHUNK_BYTES), "s_addc_u32 s35, s35, 0"]
    elif streamed:
        # the first three chunks: the current dword and the two in flight; no older vector memory operation may be counted
        pro += ["s_waitcnt vmcnt(0)", "v_mov_b32 v76, %[voff]", "s_mov_b64 s[34:35], %[strm]",
                "global_load_dwordx2 v[74:75], v76, s[34:35]",
                "global_load_dwordx2 %s, v76, s[34:35] offset:%d" % (pair(RING[0]), CHUNK_BYTES),
                "global_load_dwordx2 %s, v76, s[34:35] offset:%d" % (pair(RING[1]), 2 * CHUNK_BYTES),
                "s_add_u32 s34, s34, 0x%x" % (3 * CHUNK_BYTES), "s_addc_u32 s35, s35, 0"]
    pro += ["v_mov_b32 v78, 0", "v_mov_b32 v79, 0"] + ([] if streamed else ["v_mov_b32 v77, %[clane]"])
    if streamed:
        # s22 s23 (the op being executed: free until the first dispatch) and s28 hold first_y, first_y1, first_b1
        pro += ["s_getpc_b64 s[24:25]", ".Lpcref_%=:", "s_add_u32 s26, s24, .Lh0_%=-.Lpcref_%=", "s_addc_u32 s25, s25, 0",
                "s_movk_i32 s27, 0xfc02", "s_mov_b32 m0, 0", "s_waitcnt lgkmcnt(0)",
                "s_mov_b64 s[20:21], s[36:37]", "s_mov_b64 s[30:31], s[38:39]",
                "s_mov_b32 s22, s40", "s_mov_b32 s23, s41", "s_mov_b32 s28, s42"]
    else:
        pro += ["s_mov_b64 s[20:21], %[ops]", "s_mov_b64 s[30:31], %[mstream]", "s_movk_i32 s27, 0xfc02", "s_mov_b32 m0, 0"]
    pro += ["s_load_dwordx16 s[68:83], s[20:21], 0x0", "s_load_dwordx16 s[84:99], s[20:21], 0x40",
            "s_add_u32 s20, s20, 0x80", "s_addc_u32 s21, s21, 0",
            "s_load_dwordx16 s[36:51], s[30:31], 0x0", "s_load_dwordx16 s[52:67], s[30:31], 0x40"]
    if streamed:
        # prefetch chain start: the first observation's code is byte 0 of chunk 0, its values
        pro += ([] if held else ["s_waitcnt vmcnt(2)"]) + [
                "v_bfe_u32 v72, v74, 0, 8", "v_bfe_u32 v73, v75, 0, 8",
                "v_add_lshl_u32 v72, v72, s22, 5", "v_add_lshl_u32 v73, v73, s22, 5",
                "ds_read_b128 v[56:59], v72", "ds_read_b128 v[60:63], v72 offset:16",
                "ds_read_b128 v[64:67], v73", "ds_read_b128 v[68:71], v73 offset:16",
                # pair products: the second observation's values into buffer 1 (its byte and table are operands: a program
                # with one observation names the first again)
                ] + (lookup(BUF[1], "s28", "s23") if pairs else []) + [
                "s_waitcnt lgkmcnt(0)"]
    else:
        pro += [
            # prefetch chain start: codes of the first observation, its values, codes of the second
            "v_lshl_add_u32 v76, %[z0], 6, v77", "ds_read_u8 v74, v76", "@HALF ds_read_u8 v75, v76",
            "s_getpc_b64 s[24:25]", ".Lpcref_%=:", "s_add_u32 s26, s24, .Lh0_%=-.Lpcref_%=", "s_addc_u32 s25, s25, 0",
            "s_waitcnt lgkmcnt(0)",
            "v_add_lshl_u32 v72, v74, %[y0], 5", "v_add_lshl_u32 v73, v75, %[y0], 5",
            "ds_read_b128 v[56:59], v72", "ds_read_b128 v[60:63], v72 offset:16",
            "ds_read_b128 v[64:67], v73", "ds_read_b128 v[68:71], v73 offset:16",
            "v_lshl_add_u32 v76, %[z1], 6, v77", "ds_read_u8 v74, v76", "@HALF ds_read_u8 v75, v76",
            "s_waitcnt lgkmcnt(0)"]
    ins(pro)
    ins(RET)           # the first op
    npro = len(L)
    # ---- handlers ----
    h = pair_handlers() if pairs else handlers(streamed)
    ins([".p2align 15", ".Lh0_%=:"])
    for idx in range(NSLOTS):
        if idx:
            ins([".p2align 9"])
        ins(h.get(idx, ["s_branch .Ldone_%="]))
    ins([".p2align 9", ".Ldone_%=:"])
    W = ["%%[w%d]" % i for i in range(4)]
    if streamed:
        # the root weights: the second half of the record, into s[20:27].  The program pointer, the op, the jump target and
        # the scale constant are dead here, and no load in flight names them (the last prefetches of the matrix and of the ring
        # may still be travelling into theirs), so the one wait below serves the weights too.
        ins(["s_load_dwordx8 s[20:27], s[32:33], 0x20"])
        W = ["s[%d:%d]" % (20 + 2 * i, 21 + 2 * i) for i in range(4)]
    ins(["s_waitcnt vmcnt(0) lgkmcnt(0)"])
    # root dot product lh = w . x as one fma chain (weights 1 for no prior, 1/4 for the uniform prior: the same bits as the
    # plain sum and the scaled sum), so that only lh and the exponent leave the statement
    for (x, t) in ((XA, TA), (XB, TB)):
        ins(["v_mul_f64 %s, %s, %s" % (pair(t), W[0], pair(x))])
        for i in range(1, 4):
            ins(["v_fma_f64 %s, %s, %s, %s" % (pair(t), W[i], pair(x + 2 * i), pair(t))])
    ins(["v_mov_b32 %%[al], v%d" % TA, "v_mov_b32 %%[ah], v%d" % (TA + 1), "v_mov_b32 %%[bl], v%d" % TB, "v_mov_b32 %%[bh], v%d" % (TB + 1)])
    ins(["v_mov_b32 %[ea], v78", "v_mov_b32 %[eb], v79", "s_nop 1"])
    return L[:npro], L[npro:]


def c_string(lines):
    out = []
    for t in lines:
        if t.startswith("@HALF "):
            body = t[6:]
            out.append('        "%s offset:" #HALF "\\n\\t" \\' % body)
        elif t.endswith(":") or t.startswith(".p2align"):
            out.append('        "%s\\n" \\' % t)
        else:
            out.append('        "%s\\n\\t" \\' % t)
    return "\n".join(out)


def main():
    lines = sum(emit(), [])
    # size check: every handler must fit its slot (also checked on the object by tools/asm_layout_check.py)
    sizes = {"v_mul_f64": 8, "v_fma_f64": 8, "v_mov_b64": 4, "v_mov_b32": 4, "v_max_u32": 4, "v_max3_u32": 8, "v_lshrrev_b32": 4,
             "v_sub_u32": 8, "v_ldexp_f64": 8, "v_add3_u32": 8, "v_add_lshl_u32": 8, "v_lshl_add_u32": 8, "ds_read_b128": 8,
             "ds_read_u8": 8, "s_waitcnt": 4, "s_add_u32": 8, "s_addc_u32": 4, "s_load_dwordx16": 8, "s_setpc_b64": 4,
             "s_lshr_b32": 4, "s_and_b32": 8, "s_branch": 4, "s_movrels_b64": 4, "s_addk_i32": 4, "s_or_b32": 4, "s_mov_b32": 4,
             "v_bfe_u32": 8, "global_load_dwordx2": 8, "s_lshl_b32": 4, "s_bfe_u32": 8}
    for streamed in (False, True):
        for idx, body in handlers(streamed).items():
            n = sum(sizes[b.replace("@HALF ", "").split()[0]] for b in body)
            assert n <= HS, (streamed, idx, n)
    for idx, body in pair_handlers().items():
        assert sum(sizes[b.split()[0]] for b in body) <= HS, ("pairs", idx)
    vregs = ["v%d" % r for r in range(24, STACK0 + 64)]
    sregs = ["s%d" % r for r in range(20, 100)] + ["m0"]
    hdr = '''/* GENERATED by tools/gen_fused4_v4.py -- do not edit; change the generator and run it again.
 *
 * Assembly text of k_ll_fused4_v4 (plk_fused4_v4.h): the k = 4 pair-table interpreter with two sites per lane.  Op
 * format, handler numbering and the register map are documented in the generator. */
#ifndef PLK_FUSED4_V4_ASM_H
#define PLK_FUSED4_V4_ASM_H

#define PLK_V4_HANDLER_BYTES %d
#define PLK_V4_HANDLER_SLOTS %d
#define PLK_V4_REFILL_A %d
#define PLK_V4_REFILL_B %d

/* HALF: sites between a lane's two sites = workgroup size (an integer literal: it is pasted into ds_read offsets) */
#define PLK_V4_PROGRAM(HALF) \\
%s
        ""

#define PLK_V4_CLOBBERS "memory", "scc", "vcc", \\
        %s, \\
        %s

#endif
''' % (HS, NSLOTS, REFILL_A, REFILL_B, c_string(lines), ", ".join('"%s"' % v for v in vregs), ", ".join('"%s"' % s for s in sregs))
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "phyly_amd", "csrc", "plk_fused4_v4_asm.h")
    with open(path, "w") as f:
        f.write(hdr)
    print("wrote", path, "(%d asm lines)" % len(lines))
    # ---- streamed codes ----
    pro, lines = emit(True)
    held = emit(True, True)[0]
    assert not any(t.startswith("@HALF ") for t in pro + held + lines)
    vregs += ["v%d" % r for r in range(RING[0], RING[1] + 2)]
    hdr = '''/* GENERATED by tools/gen_fused4_v4.py -- do not edit; change the generator and run it again.
 *
 * Assembly text of k_ll_fused4_v4s (plk_fused4_v4s.h): the two-sites-per-lane interpreter with the codes streamed from
 * global memory into registers.  Op format, handler numbering and the register map are documented in the generator. */
#ifndef PLK_FUSED4_V4S_ASM_H
#define PLK_FUSED4_V4S_ASM_H

#define PLK_V4S_ADVANCE %d
#define PLK_V4S_CHUNK_BYTES %d
#define PLK_V4S_FOLD_ADV %d
#define PLK_V4S_FOLD_SCALE %d

/* prologue that requests the unit's first three chunks itself */
#define PLK_V4S_PROLOGUE \\
%s
        ""

/* prologue that takes them from the operands c0, c1, c2 */
#define PLK_V4S_PROLOGUE_HELD \\
%s
        ""

#define PLK_V4S_TABLE \\
%s
        ""

#define PLK_V4S_PROGRAM PLK_V4S_PROLOGUE PLK_V4S_TABLE
#define PLK_V4S_PROGRAM_HELD PLK_V4S_PROLOGUE_HELD PLK_V4S_TABLE

#define PLK_V4S_CLOBBERS "memory", "scc", "vcc", \\
        %s, \\
        %s

#endif
''' % (ADVANCE0, CHUNK_BYTES, FOLD_ADV0, FOLD_SCALE0, c_string(pro), c_string(held), c_string(lines), ", ".join('"%s"' % v for v in vregs), ", ".join('"%s"' % s for s in sregs))
    path = os.path.join(os.path.dirname(path), "plk_fused4_v4s_asm.h")
    with open(path, "w") as f:
        f.write(hdr)
    print("wrote", path, "(%d asm lines)" % len(pro + held + lines))
    # ---- pair products ----
    held, lines = emit(True, True, True)
    assert not any(t.startswith("@HALF ") for t in held + lines)
    hdr = '''/* GENERATED by tools/gen_fused4_v4.py -- do not edit; change the generator and run it again.
 *
 * Assembly text of k_ll_fused4_v4s<768, true, true> (plk_fused4_v4s.h): the streamed two-sites-per-lane interpreter for programs within
 * three stack slots, with two look-up buffers and PAIR ops.  Op format, handler numbering and the register map are
 * documented in the generator. */
#ifndef PLK_FUSED4_V4P_ASM_H
#define PLK_FUSED4_V4P_ASM_H

#define PLK_V4P_STACK_SLOTS %d
#define PLK_V4P_FOLD_ADV %d
#define PLK_V4P_PAIR_EVEN %d
#define PLK_V4P_PAIR_ODD %d
/* handler index of observation kind j on buffer 0, on buffer 1 (-1: none), and the kinds with an ADVANCE inside in the order of
 * their handlers; plk_v4p_obs_slot in plk_program.h states the same numbering and tests/pairmulcheck_main.cpp compares the two */
#define PLK_V4P_GEN_OBS_EVEN {%s}
#define PLK_V4P_GEN_OBS_ODD {%s}
#define PLK_V4P_GEN_OBS_FOLDED {%s}

/* the unit's first three chunks are the operands c0, c1, c2 */
#define PLK_V4P_PROGRAM_HELD \\
%s
%s
        ""

#endif
''' % (PAIR_SLOTS, PAIR_FOLD0, PAIR_EVEN0, PAIR_ODD0, ", ".join(str(v) for v in PAIR_OBS_HANDLERS),
       ", ".join(str(-1 if v is None else v) for v in PAIR_OBS_ODD), ", ".join(str(v) for v in PAIR_OBS_FOLDED), c_string(held), c_string(lines))
    path = os.path.join(os.path.dirname(path), "plk_fused4_v4p_asm.h")
    with open(path, "w") as f:
        f.write(hdr)
    print("wrote", path, "(%d asm lines)" % len(held + lines))


if __name__ == "__main__":
    main()
