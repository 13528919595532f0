"""CPU: the density screen's stream with the front end under it (tools/gen_fp16s_asm.py, cfg front=1; DESIGN 3.1 "The front end
under the stream"), on the generator's own bookkeeping: the ordinary global loads of the next pass's samples share vmcnt with
the ring's LDS-DMA, the next pass's encodings leave in a224..a255, and the MFMAs are those of the serial-front stream."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def gens():
    import gen_fp16s_asm as G
    serial = G.PassFp16s(G.nerf_sigma_layers())
    serial.generate()
    front = G.PassFp16s(G.nerf_sigma_layers(), {"front": 1})
    front.generate()
    return G, serial, front


def vm_index(g, kind, key):
    return max(i for i, op in enumerate(g.vm) if op[0] == kind and op[1] == key)


def count_of(line):
    assert line.startswith("s_waitcnt vmcnt(") and line.endswith(")")
    return int(line[len("s_waitcnt vmcnt("):-1])


def issued_before(g, line):
    """vector-memory operations of g.vm issued in front of a line of the stream (those of the pass before: all of them)"""
    return sum(1 for op in g.vm if op[2] is None or op[2] < line)


def test_the_default_stream_is_the_serial_one(gens):
    G, serial, front = gens
    assert not serial.front and not serial.front_at and not serial.load_at
    assert all(n == (G.LOOK - 2) * G.GPC for _, n in serial.boundary_wait.values())
    assert not any("global_load_dword" in ln and "lds" not in ln for ln in serial.e.lines)


def test_every_load_is_retired_by_a_counted_wait_before_its_first_use(gens):
    G, serial, g = gens
    lines = g.e.lines
    assert sorted(g.load_at) == list(range(7 * G.NCT)) and g.front_left == 0       # ts, three of the origin, three of the direction
    assert sorted(g.load_use_at) == sorted(g.load_at) == sorted(g.load_wait_at)
    for i in g.load_at:
        assert g.load_at[i] < g.load_wait_at[i] <= g.load_use_at[i], i
        assert lines[g.load_at[i]].startswith("global_load_dword") and "lds" not in lines[g.load_at[i]]
        # the wait, read back from its text: at most that many operations outstanding -- issued at the wait minus the count are
        # complete, in order, and the load is among them
        w = g.load_wait_at[i]
        done = issued_before(g, w) - count_of(lines[w])
        assert vm_index(g, "load", i) < done, i
        # nothing between the wait and the use writes the loaded register again: the next tile's load of it comes later
        later = [g.load_at[j] for j in g.load_at if lines[g.load_at[j]].split()[1] == lines[g.load_at[i]].split()[1] and g.load_at[j] > g.load_at[i]]
        assert all(g.load_use_at[i] < at for at in later), i
    # loads early, first use late: a tile's loads are MIN_LOAD_TO_USE MFMAs old at its wait
    mfma = [k for k, ln in enumerate(lines) if ln.startswith("v_mfma")]
    for c in range(G.NCT):
        mine = [i for i in g.load_at if g.load_tile[i] == c]
        assert len(mine) == 7
        first_wait = min(g.load_wait_at[i] for i in mine)
        assert sum(1 for k in mfma if max(g.load_at[i] for i in mine) < k < first_wait) >= (G.MIN_LOAD_TO_USE if c == 0 else 1)


def test_every_boundary_wait_covers_its_chunk_with_the_loads_in_flight(gens):
    G, serial, g = gens
    lines = g.e.lines
    assert sorted(g.boundary_wait) == list(range(g.padc))
    counts = set()
    for v, (at, n) in g.boundary_wait.items():
        assert count_of(lines[at]) == n <= 63 and lines[at + 1] == "s_barrier" and g.entered_at[v] == at + 1
        # chunk v + 1 has landed behind the wait: its last LDS-DMA is among the operations the count leaves complete
        done = issued_before(g, at) - n
        assert vm_index(g, "dma", v + 1) < done, v
        # ... and the wait asks for no more than that
        assert vm_index(g, "dma", v + 1) == done - 1, v
        counts.add(n)
    assert min(counts) == (G.LOOK - 2) * G.GPC < max(counts)          # some boundaries do have loads in flight behind the chunk
    # the same LDS-DMA instructions as the serial stream, chunk for chunk
    assert [op[1] for op in g.vm if op[0] == "dma"] == [op[1] for op in serial.vm if op[0] == "dma"]


def test_new_register_ranges_overlap_nothing(gens):
    G, serial, g = gens
    rm = G.register_map()
    for new in ("front_tmp", "next_keep"):
        file, first, count = rm[new]
        mine = set(range(first, first + count))
        assert max(mine) < 256
        for name, (f, a, n) in rm.items():
            if name != new and f == file:
                assert not (mine & set(range(a, a + n))), (new, name)
    assert rm["front_tmp"] == ("v", 216, 40) and rm["next_keep"] == ("a", 224, 32)


def test_next_keep_is_copied_out_then_written_once(gens):
    G, serial, g = gens
    lines = g.e.lines
    regs = list(range(G.ANEXT, G.ANEXT + 8 * G.NCT))
    assert sorted(g.copy_at) == regs == sorted(g.next_write_at)
    first_mfma = min(k for k, ln in enumerate(lines) if ln.startswith("v_mfma"))
    for j, a in enumerate(regs):
        assert lines[g.copy_at[a]] == "v_accvgpr_mov_b32 a%d, a%d" % (G.AKEEP + j, a) and g.copy_at[a] < first_mfma
        assert len(g.next_write_at[a]) == 1 and g.next_write_at[a][0] > max(g.copy_at.values())
        assert lines[g.next_write_at[a][0]].startswith("v_accvgpr_write_b32 a%d," % a)
    # and nothing else of the stream names them
    named = [k for k, ln in enumerate(lines) for a in regs if "a%d," % a in ln.replace(" ", ",") + ","]
    assert sorted(named) == sorted(list(g.copy_at.values()) + [w[0] for w in g.next_write_at.values()])


def test_mfmas_are_those_of_the_serial_stream(gens):
    G, serial, g = gens
    a = [ln for ln in serial.e.lines if ln.startswith("v_mfma")]
    b = [ln for ln in g.e.lines if ln.startswith("v_mfma")]
    assert a == b and len(a) == 968 * G.NCT
    # ... and everything else too: without the front end's own lines (its instructions, their scalar helpers and counted waits,
    # the prologue's copies in place of the writes from v88..) the stream is the serial one, but for the boundaries' counts
    own = set(g.front_at) | ({at for at, _ in g.vm_waits} - {at for at, _ in g.boundary_wait.values()})
    rest = [ln for k, ln in enumerate(g.e.lines) if k not in own and not ln.startswith(("s_mov_b32 s", "s_or_b64 vcc", "v_accvgpr_mov_b32", "s_nop 1"))]
    keep_writes = {"v_accvgpr_write_b32 a%d, v%d" % (G.AKEEP + j, G.H + j) for j in range(8 * G.NCT)}

    def blind(ln):
        return "s_waitcnt vmcnt" if ln.startswith("s_waitcnt vmcnt") else ln
    assert [blind(ln) for ln in rest] == [blind(ln) for ln in serial.e.lines if ln not in keep_writes]


def test_front_end_takes_free_gaps_one_instruction_each(gens):
    G, serial, g = gens
    lines = g.e.lines
    mfma = [k for k, ln in enumerate(lines) if ln.startswith("v_mfma")]
    import bisect
    gap_of = [bisect.bisect(mfma, k) for k in g.front_at]
    assert len(set(gap_of)) == len(gap_of) and min(gap_of) >= 1 and max(gap_of) < len(mfma)     # one a gap, all under the MFMAs
    for k, gp in zip(g.front_at, gap_of):
        gap = lines[mfma[gp - 1] + 1:mfma[gp]]
        assert not any(ln.startswith(("global_load_lds", "s_barrier", "v_pk_max_f16")) for ln in gap), gp
        assert sum(1 for ln in gap if ln.startswith("v_cvt_pk_f16_f32")) <= (1 if lines[k].startswith("v_cvt_pk_f16_f32") else 0), gp


def test_box_test_is_three_compares_per_tile_on_an_inline_constant(gens):
    """the domain rule of DESIGN 3.1 "The screen's domain": not (|p| <= BOX) per coordinate -- true of a NaN and an infinity too
    -- by the abs modifier against a float64 inline constant; the serial stream has no front end and no compare"""
    G, serial, g = gens
    lines = g.e.lines
    assert G.BOX == 2.0
    at = [k for k, ln in enumerate(lines) if ln.startswith("v_cmp_nle_f64")]
    assert len(at) == 3 * G.NCT and set(at) <= set(g.front_at)
    for c in range(G.NCT):
        a, b, d = (lines[k].replace(",", " ").split() for k in at[3 * c:3 * c + 3])
        assert (a[1], b[1], d[1]) == ("s[90:91]", "s[92:93]", "vcc") and a[3] == b[3] == d[3] == "2.0"
        regs = [x[2] for x in (a, b, d)]
        assert all(r.startswith("|v[") and r.endswith("]|") for r in regs) and len(set(regs)) == 3
    assert not any("v_cmp_class" in ln or "s86" in ln for ln in lines)
    assert not any(ln.startswith("v_cmp_nle_f64") for ln in serial.e.lines)
