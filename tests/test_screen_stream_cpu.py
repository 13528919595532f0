"""CPU: the generated instruction stream of the density screen's kernel (tools/gen_fp16s_asm.py -> csrc/fp16s_asm_nerf.inc,
csrc/mlp_nerf_fp16s.hip; DESIGN 3.1 "The screen"): the text the build wrote is current, the register map fits the two halves
of the register file, and every weight fragment is read from LDS behind the ring boundary that lands its chunk and before its first use
-- on the generator's own bookkeeping, not on the text."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def gen():
    import gen_fp16s_asm as G
    g = G.PassFp16s(G.nerf_sigma_layers())
    g.generate()
    return G, g


def test_built_stream_is_what_the_generator_emits():
    """csrc/fp16s_asm_nerf.inc is written by the Makefile at build time and kept out of git, as mx2_stash_asm_nerf.inc is: the
    file the kernel was compiled against is byte for byte what the generator emits today."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_fp16s_asm.py")], capture_output=True, text=True, check=True).stdout
    with open(os.path.join(ROOT, "tgtc-style_amd", "csrc", "fp16s_asm_nerf.inc")) as f:
        committed = f.read()
    assert out == committed, "fp16s_asm_nerf.inc is stale: make -C tgtc-style_amd/csrc"
    assert "kFp16sFrags = 968, kFp16sPadChunks = 64, kFp16sChunkBytes = 16384, kFp16sTiles = 4;" in out


def test_register_map_fits_both_halves_of_the_register_file(gen):
    G, g = gen
    used = {"v": set(), "a": set()}
    for name, (file, first, count) in G.register_map().items():
        regs = set(range(first, first + count))
        assert not (regs & used[file]), "%s overlaps another range" % name
        used[file] |= regs
    assert max(used["v"]) == G.LAST_VGPR < 256 and max(used["a"]) == G.N_AGPR - 1 < 256
    assert min(used["v"]) >= 16                     # v0..v15 stay with the compiler
    # four tiles: two layers of activations for a tile are 64 registers; sixteen weight slots of four registers
    assert G.NCT == 4 and G.register_map()["act_x"][2] == G.register_map()["act_y"][2] == 128 and G.register_map()["weights"][2] == 64


def test_every_fragment_is_read_behind_its_boundary_and_before_its_use(gen):
    G, g = gen
    assert g.nfrag == 968 and g.n_mfma == 968 * G.NCT and sorted(g.frag_op) == list(range(g.nfrag))
    assert sorted(g.entered_at) == list(range(g.padc))               # entry, every boundary, the walk to the padded end
    ops = [g.frag_op[f] for f in range(g.nfrag)]
    assert ops == sorted(ops) and len(set(ops)) == g.nfrag           # one read per fragment, in stream order
    for f in range(g.nfrag):
        ch = f // G.FPC
        assert g.op_chunk[g.frag_op[f]] == ch
        # chunks up to v + 1 have landed behind the barrier of boundary v: the read of a fragment of chunk ch follows boundary ch - 1
        assert g.entered_at[max(ch - 1, 0)] < g.read_at[f], f
        # ... and precedes boundary ch + 1, whose barrier lets the slot of chunk ch be filled again
        if ch + 1 < g.padc:
            assert g.read_at[f] < g.entered_at[ch + 1], f
        # the read is issued, then retired by a counted wait, then used
        assert g.read_at[f] < g.wait_at[f] < g.use_at[f], f
        # the slot's previous fragment has been used by then: the read-ahead distance is the number of slots
        if f >= G.NSLOT:
            assert g.use_at[f - G.NSLOT] < g.read_at[f], f
    lines = g.e.lines
    assert all(lines[g.read_at[f]].startswith("ds_read_b128 a[") for f in range(g.nfrag))
    assert all(lines[g.wait_at[f]].startswith("s_waitcnt lgkmcnt(") for f in range(g.nfrag))
    assert all(lines[g.use_at[f]].startswith("v_mfma_f32_16x16x32_f16") for f in range(g.nfrag))
    assert all(lines[g.entered_at[v]] == "s_barrier" for v in range(g.padc))
