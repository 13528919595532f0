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
            "act_x": ("v", H, NCT * 32), "weights": ("a", AW, 4 * NSLOT), "act_y": ("a", AY, NCT * 32), "keep": ("a", AKEEP, NCT * 8)}


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
        while self.dma_q and n > 0:
            self.e.emit(self.dma_q.pop(0))
            n -= 1

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
        e.emit("s_waitcnt vmcnt(%d)" % ((LOOK - 2) * GPC))
        self.entered_at[v] = len(e.lines)
        e.emit("s_barrier")
        ch = (v + LOOK) % self.padc
        slot = (v + LOOK) % SLOTS
        e.emit("s_add_u32 s96, %%[src_lo], 0x%x" % (ch * CHUNK))
        e.emit("s_addc_u32 s97, %[src_hi], 0")
        e.emit("s_add_u32 m0, %%[ldsw], 0x%x" % (slot * CHUNK))
        e.emit("s_nop 0")
        for j in range(GPC):
            self.dma_q.append("global_load_lds_dwordx4 %%[voff], s[96:97] offset:%d" % (j * 1024))
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

    # ------------------------------------------------------------------------------------------ the pass
    def generate(self):
        e = self.e
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
                e.emit("v_accvgpr_write_b32 %s, %s" % (A(AKEEP + 8 * ct + i), V(H + 8 * ct + i)))
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
                    self.drain_dma()
                    if ct == NCT - 1:
                        self.read_frag(fr + NSLOT)          # the slot is free: the fragment sixteen ahead
                        if ks == 1:
                            load_bias(grt + 2)              # the buffer was read four MFMAs ago: the row tile after the next
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
    stats = {}
    for ln in lines:
        k = ln.split()[0]
        stats[k] = stats.get(k, 0) + 1
    out.append("// pass %s: %d fragments, %d layers, %d chunks (padded %d); %d instructions; %s" % (
        name, gen.nfrag, len(layers), gen.nchunk, gen.padc, len(lines), ", ".join("%s %d" % kv for kv in sorted(stats.items(), key=lambda kv: -kv[1])[:12])))
    out.append("// keep[ct][0..1] = P[0], P[1] of column tile ct (fp16 B fragments of the point encoding), handed over in v%d..v%d and moved to" % (H, H + 8 * NCT - 1))
    out.append("// a%d..a%d by the stream; sigma[ct] (lanes 0..15) comes back in v%d..v%d.  The stream runs the whole ring protocol of one" % (AKEEP, AKEEP + 8 * NCT - 1, OUT, OUT + NCT - 1))
    out.append("// pass (entry, boundaries, walk to the padded end).")
    out.append("constexpr int kFp16sFrags = %d, kFp16sPadChunks = %d, kFp16sChunkBytes = %d, kFp16sTiles = %d;" % (gen.nfrag, gen.padc, CHUNK, NCT))
    out.append("template <class Ring>")
    out.append("__device__ __forceinline__ void fp16s_asm_%s(const Ring& ring, lds_cptr bias_lane, half8 (&keep)[%d][2], float (&sigma)[%d]) {" % (name, NCT, NCT))
    out.append("    const unsigned src_lo = __builtin_amdgcn_readfirstlane((unsigned)(size_t)ring.src[0]), src_hi = __builtin_amdgcn_readfirstlane((unsigned)((size_t)ring.src[0] >> 32));")
    out.append("    const unsigned ldsw = __builtin_amdgcn_readfirstlane((unsigned)(size_t)TGTC_LPTR(ring.lds_wave));")

    def rg(base, n):
        return "{v[%d:%d]}" % (base, base + n - 1)
    outs = ['"=&{v%d}"(sigma[%d])' % (OUT + ct, ct) for ct in range(NCT)]
    outs += ['"+%s"(keep[%d][%d])' % (rg(H + 8 * ct + 4 * i, 4), ct, i) for ct in range(NCT) for i in range(2)]
    out.append("    asm volatile(")
    out.append(block_text(lines))
    ins = ['[lane_lo] "v"(ring.lane_lo)', '[lane_hi] "v"(ring.lane_hi)', '[bias_lane] "v"(bias_lane)', '[voff] "v"(ring.voff)',
           '[src_lo] "s"(src_lo)', '[src_hi] "s"(src_hi)', '[ldsw] "s"(ldsw)']
    clob = ['"memory"', '"scc"', '"m0"', '"s96"', '"s97"']
    pinned = set(range(OUT, OUT + NCT)) | set(range(H, H + 8 * NCT))
    clob += ['"v%d"' % v for v in range(T, LAST_VGPR + 1) if v not in pinned]
    clob += ['"a%d"' % a for a in range(N_AGPR)]
    out.append("        : " + ", ".join(outs))
    out.append("        : " + ", ".join(ins))
    out.append("        : " + ", ".join(clob) + ");")
    out.append("}")
    out.append("")
    return gen


def main():
    cfg = {}
    for a in sys.argv[1:]:
        k, v = a.split("=")
        cfg[k] = int(v)
    out = ["// GENERATED by tools/gen_fp16s_asm.py %s-- do not edit; see that file for the design." % ("".join(x + " " for x in sys.argv[1:])), ""]
    emit_pass("nerf_sigma_pass", nerf_sigma_layers(), out, cfg)
    print("\n".join(out))


if __name__ == "__main__":
    main()
