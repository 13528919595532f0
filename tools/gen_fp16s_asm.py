#!/usr/bin/env python3
"""Generator of the fp16 (TGTC_PREC_FP16, one product per weight) NeRF trunk + sigma head on FOUR column tiles per wave, one
wave per SIMD: the density screen of a plain render (DESIGN 3.1 "The screen").

    tools/gen_fp16s_asm.py > tgtc-style_amd/csrc/fp16s_asm_nerf.inc      (per-sample kernel csrc/mlp_nerf_fp16s.hip; written by
                                                                          csrc/Makefile at build time, kept out of git)

The screen runs over EVERY sample of both passes.  The kernel shaped for whole fp16 networks (mlp_nerf.hip CfgFast: eight waves,
two column tiles each) reads a 1 KiB weight fragment per two MFMAs in each wave; here a fragment feeds four MFMAs, one per column
tile, which takes one wave per SIMD and the accumulator half of the register file -- so the whole pass is one generated stream,
the same move as tools/gen_x3_asm.py with one product instead of three:

  per 32-deep k-step and column tile:  acc = W.A + acc, starting from the bias   (dense_layer's order on one chain: the same bits)

  VGPR  v16..v19   sigma[ct] (outputs)                        AGPR  a0..a63     sixteen weight-fragment slots of 4 registers
        v24..v31   converted pairs on their way to AGPRs                        (ds_read straight into them; fragment f lives in
        v32..v39   the biases of two row tiles (the first                       slot f mod 16 and is read sixteen fragments -- one
                   k-step's MFMAs take them as their C operand)                 ring chunk -- ahead of its use)
        v40..v87   three accumulator sets x four tiles              a64..a191   activation set Y [tile][32] (B operand; written by
        v88..v215  activation set X [tile][32]                                  v_accvgpr_write)
                   (at entry: the encodings, copied to a192.. first) a192..a223 the point encoding's B fragments [tile][2 k-steps]

Layers alternate between the two sets (L0 writes Y, L1 reads Y and writes X, ...), so half of the activations are AGPR operands
(tools/microbench/agpr_mfma.hip: no penalty in this pattern).  The epilogue of a row tile is the fp16 store_act of mlp_core.h:
v_cvt_pk_f16_f32 of a pair, then v_pk_max_f16 with zero.

The front end under the stream (cfg front=1): while the MFMAs of pass p run, the wave loads the samples of ITS next
pass (p + gridDim.x) and encodes their points -- the arithmetic of nerf_load_samples<4, IN_RAYS> + nerf_encode<4, false, false>
(csrc/mlp_nerf_front.h), operation for operation -- with v216..v255 as temporaries, into a224..a255; the next pass's prologue
copies them to a192..a223 (v_accvgpr_mov) where the serial stream writes them from v88...  At most one front-end instruction
per MFMA gap, only in gaps that carry no epilogue filler, no LDS-DMA and no ring boundary.  The ordinary global loads count on
vmcnt with the LDS-DMA: every counted vmcnt wait of the stream -- the boundaries' and the front end's own -- is computed from
the one list of vector-memory operations in issue order (self.vm), returns being in order.

Ring protocol: as tools/gen_x3_asm.py (four waves, four LDS-DMA instructions per wave and 16 KiB chunk, one per MFMA gap; entry,
boundaries and the walk to the padded end inside the stream; the look-ahead runs into the same stream again).  A chunk holds
sixteen 1 KiB fragments here.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_mx_asm import CHUNK, LOOK, SLOTS, Emitter  # noqa: E402
from gen_x3_asm import nerf_sigma_layers  # noqa: E402

NWAVES = 4
GPC = CHUNK // (NWAVES * 1024)
NCT = 4
FRAG = 1024
FPC = CHUNK // FRAG
NSLOT = 16                     # weight-fragment register slots = the read-ahead distance in fragments

OUT = 16
T = 24
BIAS = 32
ACC = 40
H = 88
LAST_VGPR = H + NCT * 32 - 1
AW = 0
AY = AW + 4 * NSLOT
AKEEP = AY + NCT * 32
N_AGPR = AKEEP + NCT * 8
# the in-stream front end (cfg front=1): the NEXT pass's point encodings [tile][8], and its temporaries
ANEXT = N_AGPR
N_AGPR_SERIAL, N_AGPR = N_AGPR, ANEXT + NCT * 8
FT = LAST_VGPR + 1
LAST_VGPR_SERIAL, LAST_VGPR = LAST_VGPR, FT + 39
MIN_LOAD_TO_USE = 256          # MFMAs between a tile's last load and the counted wait in front of its first use (> 2 us)
FRONT_EVERY = 2                # the front end takes every second free gap: it ends in the pass's last quarter
BOX = 2.0                      # the screen's declared box |x|, |y|, |z| <= BOX (kScreenBox of csrc/mlp_nerf_mx.h): a sample outside
assert BOX in (0.5, 1.0, 2.0, 4.0)   # it gets NaN; a float64 inline constant of the compare, no literal and no register
X, Y = 0, 1                    # the activation sets of nerf_sigma_layers(): X in VGPRs, Y in AGPRs


def V(base, n=1):
    return "v%d" % base if n == 1 else "v[%d:%d]" % (base, base + n - 1)


def A(base, n=1):
    return "a%d" % base if n == 1 else "a[%d:%d]" % (base, base + n - 1)


def acc(s, ct):
    return ACC + (s * NCT + ct) * 4


def act(st, ct, ks):
    """the B operand of k-step ks, column tile ct, of activation set st"""
    return V(H + ct * 32 + 4 * ks, 4) if st == X else A(AY + ct * 32 + 4 * ks, 4)


def register_map():
    """name -> (file, first, count) of everything the stream owns"""
    return {"sigma": ("v", OUT, NCT), "pairs": ("v", T, 2 * NCT), "bias": ("v", BIAS, 8), "acc": ("v", ACC, 3 * NCT * 4),
            "act_x": ("v", H, NCT * 32), "weights": ("a", AW, 4 * NSLOT), "act_y": ("a", AY, NCT * 32), "keep": ("a", AKEEP, NCT * 8),
            "front_tmp": ("v", FT, LAST_VGPR - FT + 1), "next_keep": ("a", ANEXT, NCT * 8)}


class PassFp16s:
    def __init__(self, layers, cfg=None):
        self.layers = layers
        self.cfg = cfg or {}
        self.nfrag = sum(L.rt * L.ks for L in layers)
        self.nchunk = (self.nfrag + FPC - 1) // FPC
        self.padc = (self.nchunk + SLOTS - 1) // SLOTS * SLOTS
        self.e = Emitter()
        self.frag_op = {}            # fragment -> id of its LDS read
        self.op_chunk = {}           # LDS op -> chunk it reads
        self.dma_q = []
        self.entered = -1
        # where things stand in the stream (indices into e.lines): the checks of tests/test_screen_stream_cpu.py
        self.read_at = {}            # fragment -> its ds_read
        self.wait_at = {}            # fragment -> the counted wait that retires its read
        self.use_at = {}             # fragment -> its first MFMA
        self.entered_at = {}         # virtual chunk v -> the barrier of boundary(v): chunks up to v + 1 have landed behind it
        self.n_mfma = 0
        self.retired = 0             # fragments below this one have had their read retired
        # vector-memory operations in issue order: ("dma", virtual chunk, line) / ("load", id, line).  At entry the LOOK chunks
        # the previous pass (or the kernel's prologue) issued are in flight, and no ordinary load is younger than any of them:
        # the front end's loads are all retired inside their own pass.
        self.vm = [("dma", v, None) for v in range(LOOK) for _ in range(GPC)]
        self.vm_done = 0             # operations [0, vm_done) are known complete
        self.vm_waits = []           # (line of a counted vmcnt wait, the youngest operation it retires)
        self.boundary_wait = {}      # virtual chunk v -> (line of its counted vmcnt wait, the count)
        # the in-stream front end (cfg front=1)
        self.front = bool(self.cfg.get("front"))
        self.front_q = []            # pending items, in order: ("op", lines, loads used, AGPR written) / ("load", line, id, tile) / ("wait", tile)
        self.front_at = []           # lines of the front end's instructions placed in MFMA gaps
        self.load_at, self.load_wait_at, self.load_use_at = {}, {}, {}   # load id -> line of issue / of its wait / of its first use
        self.load_tile = {}          # load id -> tile
        self.tile_loaded_mfma = {}   # tile -> n_mfma at its last load
        self.copy_at, self.next_write_at = {}, {}    # AGPR of next_keep -> line of the prologue's copy / lines that write it
        self.free_gaps = 0

    # ------------------------------------------------------------------------------------------ vmcnt
    def vm_wait_for(self, idx):
        """the counted wait behind which operation idx of self.vm (and every older one: returns are in order) has landed"""
        n = len(self.vm) - 1 - idx
        assert 0 <= n <= 63, "vmcnt is a 6-bit counter"
        self.vm_waits.append((len(self.e.lines), idx))
        self.e.emit("s_waitcnt vmcnt(%d)" % n)
        self.vm_done = max(self.vm_done, idx + 1)
        return n

    def need(self, op):
        """Emitter.need, noting for every fragment the counted wait that retires its read"""
        e = self.e
        n0 = len(e.lines)
        e.need(op)
        if len(e.lines) > n0:
            while self.retired < self.nfrag and self.frag_op.get(self.retired) is not None and self.frag_op[self.retired] < e.lds_done:
                self.wait_at[self.retired] = n0
                self.retired += 1

    # ------------------------------------------------------------------------------------------ ring
    def drain_dma(self, n=1):
        did = 0
        while self.dma_q and n > 0:
            text, v = self.dma_q.pop(0)
            self.vm.append(("dma", v, len(self.e.lines)))
            self.e.emit(text)
            n -= 1
            did += 1
        return did

    def boundary(self, v):
        e = self.e
        self.drain_dma(99)
        # reads of the chunk whose slot is re-filled (v-1) must have returned in THIS wave before it joins the barrier
        victims = [op for op, ch in self.op_chunk.items() if ch <= v - 1 and op >= e.lds_done]
        if victims:
            self.need(max(victims))
        if self.cfg.get("abl_ring"):             # timing experiment: no counted wait, barrier or LDS-DMA
            self.entered_at[v] = len(e.lines)
            self.entered = v
            return
        # chunk v + 1 lands here: behind its last LDS-DMA the wave has issued those of LOOK - 2 chunks, and whatever ordinary
        # loads of the front end came after it
        at = len(e.lines)
        n = self.vm_wait_for(max(i for i, op in enumerate(self.vm) if op[0] == "dma" and op[1] == v + 1))
        assert self.front or n == (LOOK - 2) * GPC
        self.boundary_wait[v] = (at, n)
        self.entered_at[v] = len(e.lines)
        e.emit("s_barrier")
        ch = (v + LOOK) % self.padc
        slot = (v + LOOK) % SLOTS
        e.emit("s_add_u32 s96, %%[src_lo], 0x%x" % (ch * CHUNK))
        e.emit("s_addc_u32 s97, %[src_hi], 0")
        e.emit("s_add_u32 m0, %%[ldsw], 0x%x" % (slot * CHUNK))
        e.emit("s_nop 0")
        for j in range(GPC):
            self.dma_q.append(("global_load_lds_dwordx4 %%[voff], s[96:97] offset:%d" % (j * 1024), v + LOOK))
        self.entered = v

    def acquire_for(self, f):
        """enter the chunk fragment f lies in (chunks up to entered + 1 are readable)"""
        want = min(f, self.nfrag - 1) // FPC - 1
        while self.entered < want:
            self.boundary(self.entered + 1)

    def read_frag(self, f):
        if f >= self.nfrag:
            return
        e = self.e
        self.acquire_for(f)
        if self.cfg.get("abl_reads") and f >= NSLOT:      # timing experiment: no weight reads behind the first sixteen
            self.frag_op[f] = None
            return
        ch = f // FPC
        assert ch - 1 <= self.entered
        off = (ch % SLOTS) * CHUNK + (f % FPC) * FRAG
        base = "%[lane_lo]" if off < 65536 else "%[lane_hi]"
        self.read_at[f] = len(e.lines)
        op = e.lds("ds_read_b128 %s, %s offset:%d" % (A(AW + 4 * (f % NSLOT), 4), base, off % 65536))
        self.op_chunk[op] = ch
        self.frag_op[f] = op

    # ------------------------------------------------------------------------------------------ epilogue (store_act, fp16)
    def epi_ops(self, rt, st, s):
        e = self.e
        ks = rt // 2
        body = [[] for _ in range(NCT)]
        for ct in range(NCT):
            a = acc(s, ct)
            for half in range(2):
                d = 4 * ks + (rt & 1) * 2 + half
                a0, a1 = a + 2 * half, a + 2 * half + 1
                ops = body[ct]
                if st == X:
                    h = H + ct * 32 + d
                    ops.append(lambda h=h, a0=a0, a1=a1: e.emit("v_cvt_pk_f16_f32 %s, %s, %s" % (V(h), V(a0), V(a1))))
                    ops.append(lambda h=h: e.emit("v_pk_max_f16 %s, %s, 0" % (V(h), V(h))))
                else:
                    t, y = T + 2 * ct + half, AY + ct * 32 + d
                    ops.append(lambda t=t, a0=a0, a1=a1: e.emit("v_cvt_pk_f16_f32 %s, %s, %s" % (V(t), V(a0), V(a1))))
                    ops.append(lambda t=t: e.emit("v_pk_max_f16 %s, %s, 0" % (V(t), V(t))))
                    ops.append(lambda t=t, y=y: e.emit("v_accvgpr_write_b32 %s, %s" % (A(y), V(t))))
        merged = []
        for i in range(max(len(b) for b in body)):
            for ct in range(NCT):
                if i < len(body[ct]):
                    merged.append(body[ct][i])
        return merged

    # ------------------------------------------------------------------------------------------ the front end under the stream
    def front_items(self):
        """The next pass's samples and point encodings: nerf_load_samples<4, IN_RAYS> and nerf_encode<4, false, false> of
        csrc/mlp_nerf_front.h for this wave's 4 x 16 samples from %[snext] on, the same IEEE operations per value in the same
        order (float64 FMA of o + t.d, x kInv2Pi, ldexp by the band, rint, subtract, convert, v_sin / v_cos in turns, packed
        convert to fp16).  Lane n + 16 g holds sample n of a tile for lane group g, which owns pairs q = 8 g + i: pair i is
        coordinate (2 g + i) mod 3 -- the lane loads the three coordinates rotated by 2 g mod 3, so that pair i reads
        rotated coordinate i mod 3 in every lane -- at band (8 g + i) / 3, a nibble of a per-lane constant.  Lane group 3
        (rotation 0) replaces pairs 6 and 7 by the raw (x, y), (z, 0).
        Scalars the stream owns: s[84:85] lanes 48..63, s87 a literal on its way, s[88:89] kInv2Pi, s[90:93] compare
        results."""
        t = FT
        NBAD, BANDS, ROT, N16, S, RR, Q = t, t + 1, (t + 2, t + 3, t + 4), t + 5, t + 6, t + 7, t + 8
        TS, AD, AD2 = t + 9, t + 10, t + 12
        O, D, P, RAW = t + 14, t + 20, t + 26, t + 32
        F, TA, TB = t + 35, t + 36, t + 38
        SX, CX, PK, T1 = TB, TB + 1, TA, TA + 1        # (the float32 tail of a pair runs in the registers of its float64 head)
        assert TB + 1 == LAST_VGPR and not any(r & 1 for r in (t, AD, AD2, O, D, P, TA, TB)), "64-bit tuples are even-aligned"
        q = self.front_q
        lid = [0]

        def op(*lines, uses=(), writes=None):
            q.append(("op", list(lines), tuple(uses), writes))

        def load(line, tile):
            q.append(("load", line, lid[0], tile))
            lid[0] += 1
            return lid[0] - 1

        def v2(r):
            return V(r, 2)

        # per-lane constants of the pass
        op("v_mbcnt_lo_u32_b32 %s, -1, 0" % V(S))
        op("v_mbcnt_hi_u32_b32 %s, -1, %s" % (V(S), V(S)))
        op("v_and_b32 %s, 15, %s" % (V(N16), V(S)))
        op("v_lshrrev_b32 %s, 4, %s" % (V(Q), V(S)))
        op("v_lshlrev_b32 %s, 3, %s" % (V(Q), V(Q)))
        for k, lit in enumerate((0x00081000, 0x08100008, 0x10000810)):      # byte g: 8 ((2 g + k) mod 3)
            assert all((lit >> (8 * g)) & 255 == 8 * ((2 * g + k) % 3) for g in range(4))
            op("s_mov_b32 s87, 0x%08x" % lit, "v_bfe_u32 %s, s87, %s, 8" % (V(ROT[k]), V(Q)))
        bands = [sum(((8 * g + i) // 3) << (4 * i) for i in range(8)) for g in range(4)]
        op("v_mov_b32 %s, 0x%08x" % (V(BANDS), bands[0]))
        for g, (lo, hi) in ((1, (0xffff0000, 0)), (2, (0, 0x0000ffff)), (3, (0, 0xffff0000))):
            op("v_mov_b32 %s, 0x%08x" % (V(T1), bands[g]))
            op("s_mov_b32 s90, 0x%08x" % lo, "s_mov_b32 s91, 0x%08x" % hi, "v_cndmask_b32_e64 %s, %s, %s, s[90:91]" % (V(BANDS), V(BANDS), V(T1)))

        def part_a(c):
            """sample index (clamped to M - 1 as nerf_load_samples clamps it), ray = index / N (the exact 32-bit division by a
            reciprocal word: quotient estimate, two refinements), addresses, seven loads"""
            op("v_add3_u32 %s, %%[snext], %s, %d" % (V(S), V(N16), 16 * c))
            op("v_min_u32 %s, %%[mm1], %s" % (V(S), V(S)))
            op("v_mul_hi_u32 %s, %s, %%[zz]" % (V(Q), V(S)))
            op("v_mul_lo_u32 %s, %s, %%[nn]" % (V(RR), V(Q)))
            op("v_sub_u32 %s, %s, %s" % (V(RR), V(S), V(RR)))
            for _ in range(2):
                op("v_cmp_le_u32 vcc, %%[nn], %s" % V(RR))
                op("v_subrev_u32 %s, %%[nn], %s" % (V(T1), V(RR)))
                op("v_cndmask_b32 %s, %s, %s, vcc" % (V(RR), V(RR), V(T1)))
                op("v_addc_co_u32 %s, vcc, 0, %s, vcc" % (V(Q), V(Q)))
            ids = {}
            op("v_mad_u64_u32 %s, vcc, %s, 4, %%[ts]" % (v2(AD), V(S)))
            ids["ts"] = load("global_load_dword %s, %s, off" % (V(TS), v2(AD)), c)
            for name, base, ptr in (("o", O, "ro"), ("d", D, "rd")):
                op("v_mad_u64_u32 %s, vcc, %s, 24, %%[%s]" % (v2(AD), V(Q), ptr))
                for k in range(3):
                    op("v_add_co_u32 %s, vcc, %s, %s" % (V(AD2), V(ROT[k]), V(AD)))
                    op("v_addc_co_u32 %s, vcc, 0, %s, vcc" % (V(AD2 + 1), V(AD + 1)))
                    ids[name, k] = load("global_load_dwordx2 %s, %s, off" % (v2(base + 2 * k), v2(AD2)), c)
            return ids

        ids = part_a(0)
        for c in range(NCT):
            q.append(("wait", c))
            op("v_cvt_f64_f32 %s, %s" % (v2(TA), V(TS)), uses=[ids["ts"]])
            for k in range(3):
                op("v_fma_f64 %s, %s, %s, %s" % (v2(P + 2 * k), v2(TA), v2(D + 2 * k), v2(O + 2 * k)), uses=[ids["o", k], ids["d", k]])
            if c + 1 < NCT:
                ids = part_a(c + 1)          # the loaded registers are free: the next tile's loads fly under this tile's encoding
            # position outside the screen's box -> bit c of NBAD: not (|p| <= BOX) per coordinate, true of a NaN and of an
            # infinity as well; BOX is a float64 inline constant
            op("v_cmp_nle_f64 s[90:91], |%s|, %s" % (v2(P), BOX))
            op("v_cmp_nle_f64 s[92:93], |%s|, %s" % (v2(P + 2), BOX))
            op("v_cmp_nle_f64 vcc, |%s|, %s" % (v2(P + 4), BOX))
            op("s_or_b64 vcc, vcc, s[90:91]", "s_or_b64 vcc, vcc, s[92:93]", "v_cndmask_b32_e64 %s, 0, %d, vcc" % (V(NBAD if c == 0 else T1), 1 << c))
            if c:
                op("v_or_b32 %s, %s, %s" % (V(NBAD), V(NBAD), V(T1)))
            for k in range(3):
                op("v_cvt_f32_f64 %s, %s" % (V(RAW + k), v2(P + 2 * k)))
            for k in range(3):
                op("v_mul_f64 %s, %s, s[88:89]" % (v2(P + 2 * k), v2(P + 2 * k)))
            for i in range(8):
                op("v_bfe_u32 %s, %s, %d, 4" % (V(T1), V(BANDS), 4 * i))
                op("v_ldexp_f64 %s, %s, %s" % (v2(TA), v2(P + 2 * (i % 3)), V(T1)))
                op("v_rndne_f64 %s, %s" % (v2(TB), v2(TA)))
                op("v_add_f64 %s, %s, -%s" % (v2(TA), v2(TA), v2(TB)))
                op("v_cvt_f32_f64 %s, %s" % (V(F), v2(TA)))
                op("v_sin_f32 %s, %s" % (V(SX), V(F)))
                op("v_cos_f32 %s, %s" % (V(CX), V(F)))
                if i >= 6:                   # lane group 3: the raw pairs 30 (x, y) and 31 (z, 0)
                    op("v_cndmask_b32_e64 %s, %s, %s, s[84:85]" % (V(SX), V(SX), V(RAW + 2 * (i - 6))))
                    op("v_cndmask_b32_e64 %s, %s, %s, s[84:85]" % (V(CX), V(CX), V(RAW + 1) if i == 6 else "0"))
                op("v_cvt_pk_f16_f32 %s, %s, %s" % (V(PK), V(SX), V(CX)))
                op("v_accvgpr_write_b32 %s, %s" % (A(ANEXT + 8 * c + i), V(PK)), writes=ANEXT + 8 * c + i)

    def front_step(self, force=False):
        """one item of the front end into this gap (a counted wait shares the gap of the instruction it guards)"""
        e = self.e
        q = self.front_q
        if not q:
            return
        if q[0][0] == "wait":
            c = q[0][1]
            if not force and self.n_mfma < self.tile_loaded_mfma[c] + MIN_LOAD_TO_USE:
                return
            mine = [i for i, o in enumerate(self.vm) if o[0] == "load" and self.load_tile[o[1]] == c]
            if max(mine) >= self.vm_done:    # (or a ring boundary's wait has retired them already)
                self.vm_wait_for(max(mine))
            for i in mine:
                self.load_wait_at[self.vm[i][1]] = min(at for at, upto in self.vm_waits if upto >= i)
            q.pop(0)
        it = q.pop(0)
        # gfx950: two wait states between a VALU write of vcc or an SGPR and a VALU read of it (hipcc's s_nop 1); consecutive
        # front-end instructions are FRONT_EVERY free gaps apart, two MFMAs or more -- but in a flush behind the last MFMA
        if self.front_at and len(e.lines) - self.front_at[-1] - 1 < 2:
            e.emit("s_nop 1")
        if it[0] == "load":
            _, line, i, c = it
            self.load_at[i] = len(e.lines)
            self.load_tile[i] = c
            self.vm.append(("load", i, len(e.lines)))
            self.tile_loaded_mfma[c] = self.n_mfma
            self.front_at.append(len(e.lines))
            e.emit(line)
            return
        _, lines, uses, writes = it
        for i in uses:
            self.load_use_at.setdefault(i, len(e.lines))
        for ln in lines:
            if ln.startswith("v_"):
                self.front_at.append(len(e.lines))
                if writes is not None:
                    self.next_write_at.setdefault(writes, []).append(len(e.lines))
            e.emit(ln)

    # ------------------------------------------------------------------------------------------ the pass
    def generate(self):
        e = self.e
        if self.front:
            self.front_items()
        rows = []                    # (layer index, rt, first fragment)
        f = 0
        bias0 = 0
        for li, L in enumerate(self.layers):
            L.bias0 = bias0
            bias0 += 16 * L.rt
            for rt in range(L.rt):
                rows.append((li, rt, f))
                f += L.ks
        assert f == self.nfrag
        total_rt = len(rows)
        bias_op = {}

        def load_bias(grt):
            """the bias of row tile grt into its buffer (grt mod 2): its last readers were the first k-step's MFMAs of row tile grt - 2"""
            if grt >= total_rt:
                return
            li, rt, _ = rows[grt]
            boff = self.layers[li].bias0 + 16 * rt
            bias_op[grt] = e.lds("ds_read_b128 %s, %%[bias_lane] offset:%d" % (V(BIAS + 4 * (grt % 2), 4), boff * 4))

        fillers = []
        tail_of = [None]             # (set, k-step) the pending fillers still have to complete

        def run_filler():
            fl = fillers.pop(0)
            if not self.cfg.get("abl_epi"):
                fl()

        def flush(gap=99):
            # the fillers start by reading the previous row tile's accumulators: fewer than four MFMAs behind its last one the
            # result is not there yet -- drain explicitly
            if fillers and gap < 4:
                e.emit("s_nop 7")
                e.emit("s_nop 7")
            while fillers:
                run_filler()
            tail_of[0] = None

        def epilogue(grt):
            li, rt, _ = rows[grt]
            L = self.layers[li]
            s = grt % 3
            if L.sink == "sigma":
                return [lambda ct=ct: e.emit("v_mov_b32_e32 %s, %s" % (V(OUT + ct), V(acc(s, ct)))) for ct in range(NCT)]
            return self.epi_ops(rt, L.sink, s)

        # ---- prologue: the encodings to their AGPRs, enter the pass, biases of two row tiles, the first NSLOT fragments
        for ct in range(NCT):
            for i in range(8):
                if self.front:               # what the previous pass's stream (or the kernel's prologue) left in next_keep
                    self.copy_at[ANEXT + 8 * ct + i] = len(e.lines)
                    e.emit("v_accvgpr_mov_b32 %s, %s" % (A(AKEEP + 8 * ct + i), A(ANEXT + 8 * ct + i)))
                else:
                    e.emit("v_accvgpr_write_b32 %s, %s" % (A(AKEEP + 8 * ct + i), V(H + 8 * ct + i)))
        if self.front:
            for r, lit in ((84, 0), (85, 0xffff0000), (88, 0x6dc9c883), (89, 0x3fc45f30)):
                e.emit("s_mov_b32 s%d, 0x%08x" % (r, lit))
        self.boundary(0)
        self.drain_dma(99)
        for r in range(2):
            load_bias(r)
        for f0 in range(NSLOT):
            self.read_frag(f0)
            self.drain_dma(99)

        f16 = "v_mfma_f32_16x16x32_f16 %s, %s, %s, %s"
        for grt, (li, rt, f0) in enumerate(rows):
            L = self.layers[li]
            s = grt % 3
            if grt > 0:
                pli, prt, _ = rows[grt - 1]
                PL = self.layers[pli]
                fillers.extend(epilogue(grt - 1))
                if isinstance(PL.sink, int):
                    tail_of[0] = (PL.sink, prt // 2)
            n_row = L.ks * NCT
            gap = 0
            for ks in range(L.ks):
                fr = f0 + ks
                is_act = ks < L.act
                if is_act and tail_of[0] == (L.src, ks):
                    flush(gap)
                # one counted wait per PAIR of fragments: with sixteen fragments read ahead the next one landed long ago, and a
                # wait is an instruction the lone wave has to issue like any other
                ops_needed = [self.frag_op[fr]] if self.frag_op.get(fr) is not None else []
                if fr % 2 == 0 and self.frag_op.get(fr + 1) is not None:
                    ops_needed.append(self.frag_op[fr + 1])
                if ks == 0:
                    ops_needed.append(bias_op[grt])
                if ops_needed:
                    self.need(max(ops_needed))
                w = A(AW + 4 * (fr % NSLOT), 4)
                self.use_at[fr] = len(e.lines)
                for ct in range(NCT):
                    a = V(acc(s, ct), 4)
                    c_in = V(BIAS + 4 * (grt % 2), 4) if ks == 0 else a
                    b = act(L.src, ct, ks) if is_act else A(AKEEP + 8 * ct + 4 * (ks - L.act), 4)
                    e.emit(f16 % (a, w, b, c_in))
                    self.n_mfma += 1
                    was = self.entered
                    busy = self.drain_dma() > 0
                    if ct == NCT - 1:
                        self.read_frag(fr + NSLOT)          # the slot is free: the fragment sixteen ahead
                        if ks == 1:
                            load_bias(grt + 2)              # the buffer was read four MFMAs ago: the row tile after the next
                    busy = busy or self.entered != was or (gap >= 3 and bool(fillers))
                    if not busy:                            # a free gap: no LDS-DMA, no ring boundary, no epilogue filler
                        self.free_gaps += 1
                        if self.free_gaps % self.cfg.get("front_every", FRONT_EVERY) == 0:
                            self.front_step()
                    if gap >= 3 and fillers:
                        remaining = max(n_row - 1 - gap, 0) + 1
                        if tail_of[0] is not None and tail_of[0][0] == L.src and tail_of[0][1] < L.act:
                            first_dep = tail_of[0][1] * NCT
                            remaining = max(first_dep - 1 - gap, 0) + 1
                        n = (len(fillers) + remaining - 1) // remaining
                        for _ in range(n):
                            if fillers:
                                run_filler()
                    gap += 1
            assert not fillers, "a row tile's epilogue finishes within the next row tile"
            tail_of[0] = None
        e.emit("s_nop 7")
        e.emit("s_nop 7")
        fillers.extend(epilogue(total_rt - 1))
        flush()
        self.front_left = sum(1 for it in self.front_q if it[0] != "wait")      # (0 but in the timing experiments)
        while self.front_q:
            self.front_step(force=True)
        e.emit("s_waitcnt lgkmcnt(0)")
        e.lds_done = e.lds_issued
        for v in range(self.entered + 1, self.padc):
            self.boundary(v)
        self.drain_dma(99)
        return e.lines


def block_text(lines):
    return "\n".join('        "%s\\n\\t"' % ln for ln in lines)


def emit_pass(name, layers, out, cfg=None):
    gen = PassFp16s(layers, cfg)
    lines = gen.generate()
    front = gen.front
    stats = {}
    for ln in lines:
        k = ln.split()[0]
        stats[k] = stats.get(k, 0) + 1
    out.append("// pass %s: %d fragments, %d layers, %d chunks (padded %d); %d instructions; %s" % (
        name, gen.nfrag, len(layers), gen.nchunk, gen.padc, len(lines), ", ".join("%s %d" % kv for kv in sorted(stats.items(), key=lambda kv: -kv[1])[:12])))
    if front:
        out.append("// The stream with the front end under it: P[0], P[1] of the four column tiles of THIS pass come in a%d..a%d and are copied to" % (ANEXT, N_AGPR - 1))
        out.append("// a%d..a%d; the same of the wave's next pass (samples snext + 16 ct + (lane & 15), clamped to mm1 = M - 1; nn = N, zz = its" % (AKEEP, AKEEP + 8 * NCT - 1))
        out.append("// reciprocal word, udiv_word()) leave in them, with bit ct of nbad set where a position is outside the box.  a%d..a%d are no operands:" % (ANEXT, N_AGPR - 1))
        out.append("// as operands hipcc carries them through the loop in VGPRs, 64 copies a pass.  They are clobbers of both statements, which")
        out.append("// makes them part of the kernel's allocation and keeps values of the compiler's out of them; the HIP code between two")
        out.append("// passes (sixteen lanes' stores) has no use for an AGPR.  %d front-end instructions in %d of the %d free MFMA gaps, %d" % (
            len(gen.front_at), len(gen.front_at) - gen.front_left, gen.free_gaps, gen.front_left))
        out.append("// behind the last MFMA.")
        out.append("__device__ __forceinline__ void fp16s_asm_first_keep(const half8 (&keep)[%d][2]) {" % NCT)
        out.append("    typedef unsigned word4 __attribute__((ext_vector_type(4)));")
        for ct in range(NCT):
            out.append("    asm volatile(")
            out.append(block_text(["v_accvgpr_write_b32 a%d, %%%d" % (ANEXT + 8 * ct + j, j) for j in range(8)]))
            out.append("        :")
            out.append("        : " + ", ".join('"v"(__builtin_bit_cast(word4, keep[%d][%d])[%d])' % (ct, j // 4, j % 4) for j in range(8)))
            out.append("        : " + ", ".join('"a%d"' % a for a in range(ANEXT + 8 * ct, ANEXT + 8 * ct + 8)) + ");")
        out.append("}")
        out.append("")
        out.append("template <class Ring>")
        out.append("__device__ __forceinline__ void fp16s_asm_%s(const Ring& ring, lds_cptr bias_lane, float (&sigma)[%d], unsigned& nbad," % (name, NCT))
        out.append("        const float* ts, const double* ro, const double* rd, unsigned mm1, unsigned nn, unsigned zz, unsigned snext) {")
    else:
        out.append("// keep[ct][0..1] = P[0], P[1] of column tile ct (fp16 B fragments of the point encoding), handed over in v%d..v%d and moved to" % (H, H + 8 * NCT - 1))
        out.append("// a%d..a%d by the stream; sigma[ct] (lanes 0..15) comes back in v%d..v%d.  The stream runs the whole ring protocol of one" % (AKEEP, AKEEP + 8 * NCT - 1, OUT, OUT + NCT - 1))
        out.append("// pass (entry, boundaries, walk to the padded end).")
        out.append("constexpr int kFp16sFrags = %d, kFp16sPadChunks = %d, kFp16sChunkBytes = %d, kFp16sTiles = %d;" % (gen.nfrag, gen.padc, CHUNK, NCT))
        out.append("constexpr double kFp16sBox = %s;   // the box the in-stream front end tests positions against (kScreenBox)" % BOX)
        out.append("template <class Ring>")
        out.append("__device__ __forceinline__ void fp16s_asm_%s(const Ring& ring, lds_cptr bias_lane, half8 (&keep)[%d][2], float (&sigma)[%d]) {" % (name, NCT, NCT))
    out.append("    const unsigned src_lo = __builtin_amdgcn_readfirstlane((unsigned)(size_t)ring.src[0]), src_hi = __builtin_amdgcn_readfirstlane((unsigned)((size_t)ring.src[0] >> 32));")
    out.append("    const unsigned ldsw = __builtin_amdgcn_readfirstlane((unsigned)(size_t)TGTC_LPTR(ring.lds_wave));")

    def rg(base, n):
        return "{v[%d:%d]}" % (base, base + n - 1)
    outs = ['"=&{v%d}"(sigma[%d])' % (OUT + ct, ct) for ct in range(NCT)]
    ins = ['[lane_lo] "v"(ring.lane_lo)', '[lane_hi] "v"(ring.lane_hi)', '[bias_lane] "v"(bias_lane)', '[voff] "v"(ring.voff)',
           '[src_lo] "s"(src_lo)', '[src_hi] "s"(src_hi)', '[ldsw] "s"(ldsw)']
    clob = ['"memory"', '"scc"', '"m0"', '"s96"', '"s97"']
    if front:
        outs.append('"=&{v%d}"(nbad)' % FT)
        ins += ['[ts] "s"(ts)', '[ro] "s"(ro)', '[rd] "s"(rd)', '[mm1] "s"(mm1)', '[nn] "s"(nn)', '[zz] "s"(zz)', '[snext] "s"(snext)']
        clob += ['"vcc"'] + ['"s%d"' % r for r in range(84, 94)]
        pinned = set(range(OUT, OUT + NCT)) | {FT}
        clob += ['"v%d"' % v for v in range(T, LAST_VGPR + 1) if v not in pinned]
        clob += ['"a%d"' % a for a in range(N_AGPR)]
    else:
        outs += ['"+%s"(keep[%d][%d])' % (rg(H + 8 * ct + 4 * i, 4), ct, i) for ct in range(NCT) for i in range(2)]
        pinned = set(range(OUT, OUT + NCT)) | set(range(H, H + 8 * NCT))
        clob += ['"v%d"' % v for v in range(T, LAST_VGPR_SERIAL + 1) if v not in pinned]
        clob += ['"a%d"' % a for a in range(N_AGPR_SERIAL)]
    out.append("    asm volatile(")
    out.append(block_text(lines))
    out.append("        : " + ", ".join(outs))
    out.append("        : " + ", ".join(ins))
    out.append("        : " + ", ".join(clob) + ");")
    out.append("}")
    out.append("")
    return gen


def main():
    """both streams of the kernel: the serial-front one (the first pass of a workgroup's, and the yardstick) and the one with
    the front end under it; k=v arguments are the timing experiments' switches, for both"""
    cfg = {}
    for a in sys.argv[1:]:
        k, v = a.split("=")
        cfg[k] = int(v)
    out = ["// GENERATED by tools/gen_fp16s_asm.py %s-- do not edit; see that file for the design." % ("".join(x + " " for x in sys.argv[1:])), ""]
    emit_pass("nerf_sigma_pass", nerf_sigma_layers(), out, dict(cfg, front=0))
    gen = emit_pass("nerf_sigma_pass_front", nerf_sigma_layers(), out, dict(cfg, front=1))
    assert gen.front_left == 0 or any(k.startswith("abl_") for k in cfg), "the front end must end under the MFMAs"
    print("\n".join(out))


if __name__ == "__main__":
    main()
