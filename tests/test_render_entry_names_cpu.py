"""CPU: every entry point of csrc/render.hip that is a thin wrapper around a body it shares with its siblings -- the three
culled renders, the six restyles, the two trunk builders, the two folded list launches -- reports its errors under ITS OWN name
and applies ITS OWN rule for the handles' precisions.  A wrapper that hands the shared body a sibling's name or flags fails here.

Everything asserted is returned before a device is touched: null handles, and the fake handles of test_restyle_mx_cpu (zeroed
memory behind the handle's kind and precision, without mx streams)."""
import ctypes

import pytest

from test_restyle_mx_cpu import fake_handle

ERR_ARG, ERR_UNSUPPORTED = -1, -2
KIND_NERF, KIND_STYLE = 0, 1
PREC_FP16X3, PREC_FP16_FP6 = 0, 2
BIG = 1 << 40                        # any buffer size: no call gets as far as comparing it
_BUF = (ctypes.c_char * 4096)()
P = ctypes.addressof(_BUF)           # stands for any non-null pointer: the calls must return before they read through it


# family -> (the leading handles, takes a K, the arguments after the handles); n = n_coarse = n_fine, or N / 2
FAMILIES = {
    "culled": (("coarse", "nerf", "style"), True,
               lambda K, R, n, count: (P, P, P, K, R, n, n, 0.0, 1.0, None, 0.0, P, BIG, P, P, P, None)),
    "list_restyle": (("nerf", "style"), True, lambda K, R, n, count: (P, P, P, K, R, n, n, P, BIG, count, P, BIG, P, P, None)),
    "plane_restyle": (("style",), True, lambda K, R, n, count: (P, P, P, K, R, n, n, P, BIG, count, P, BIG, P, BIG, P, P, None)),
    "trunk": (("nerf",), False, lambda K, R, n, count: (P, P, R, n, n, P, BIG, count, P, BIG, None)),
    "folded_list": (("nerf", "style"), True, lambda K, R, n, count: (P, P, P, P, K, R, 2 * n, P, P, P, None)),
}
# entry -> (family, the precision of the NeRF handle it takes, its rule: "same", "list_mx", "plane_mx" or None)
ENTRIES = {
    "tgtc_render_rays_styled_sparse": ("culled", PREC_FP16X3, "same"),
    "tgtc_render_rays_styled_sparse_folded": ("culled", PREC_FP16X3, "same"),
    "tgtc_render_rays_styled_sparse_folded_mx": ("culled", PREC_FP16_FP6, "list_mx"),
    "tgtc_restyle_rays": ("list_restyle", PREC_FP16X3, "same"),
    "tgtc_restyle_rays_folded": ("list_restyle", PREC_FP16X3, "same"),
    "tgtc_restyle_rays_folded_mx": ("list_restyle", PREC_FP16_FP6, "list_mx"),
    "tgtc_restyle_rays_trunk": ("plane_restyle", None, None),
    "tgtc_restyle_rays_trunk_folded": ("plane_restyle", None, None),
    "tgtc_restyle_rays_trunk_folded_mx": ("plane_restyle", None, "plane_mx"),
    "tgtc_geometry_trunk": ("trunk", PREC_FP16X3, None),
    "tgtc_geometry_trunk_mx": ("trunk", PREC_FP16_FP6, None),
    "tgtc_styled_forward_list_folded": ("folded_list", PREC_FP16X3, "same"),
    "tgtc_styled_forward_list_folded_mx": ("folded_list", PREC_FP16_FP6, "list_mx"),
}


class _Entry:
    """One entry point, with handles whose kinds and precisions it accepts: an fp16x3 coarse handle, the fine / nerf handle
    in the precision ENTRIES names, an fp16x3 style handle without mx streams."""

    def __init__(self, name):
        from tgtc_style_amd import hip
        self.lib, self.name = hip.load(), name
        family, nerf_precision, self.rule = ENTRIES[name]
        self.roles, self.takes_K, self.rest = FAMILIES[family]
        self.n_handles = len(self.roles)
        self.prefix = name[len("tgtc_"):].encode() + b":"
        self.keep = []
        self.handles = self.make(nerf_precision)

    def make(self, nerf_precision):
        """The leading handles as addresses, the fine / nerf handle in `nerf_precision`."""
        made = {"coarse": fake_handle(KIND_NERF, PREC_FP16X3), "nerf": fake_handle(KIND_NERF, nerf_precision or PREC_FP16X3),
                "style": fake_handle(KIND_STYLE, PREC_FP16X3)}
        self.keep.append(made)
        return [ctypes.addressof(made[role]) for role in self.roles]

    def __call__(self, handles=None, K=2, R=4, n=64, count=10):
        handles = self.handles if handles is None else handles
        return getattr(self.lib, self.name)(*handles, *self.rest(K, R, n, count))

    def error(self):
        return self.lib.tgtc_last_error()

    def named(self):
        """Does the last error begin with this entry's own name (without tgtc_) and a colon?"""
        return self.error().startswith(self.prefix)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_range_errors_carry_the_entrys_own_name(name):
    e = _Entry(name)
    if e.takes_K:
        assert e(K=0) == ERR_ARG and e.named() and b"K >= 1" in e.error(), e.error()
    assert e(R=-1) == ERR_ARG and e.named(), e.error()
    # R x (n_coarse + n_fine) = 2^24 x 128 = 2^31 exactly
    assert e(R=1 << 24) == ERR_UNSUPPORTED and e.named() and b"2^31" in e.error(), e.error()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_null_handles_are_named_as_such_under_the_entrys_own_name(name):
    e = _Entry(name)
    assert e(handles=[None] * e.n_handles) == ERR_ARG and e.named() and b"null handle" in e.error(), e.error()
    # ... and so is a single one (the last: the style handle, or the only handle)
    assert e(handles=e.handles[:-1] + [None]) == ERR_ARG and e.named() and b"null handle" in e.error(), e.error()


@pytest.mark.parametrize("name", sorted(n for n, v in ENTRIES.items() if v[2] == "same"))
def test_same_precision_entries_refuse_the_mixed_pair(name):
    e = _Entry(name)
    assert e(handles=e.make(PREC_FP16_FP6)) == ERR_ARG and e.named() and b"different precisions" in e.error(), e.error()


@pytest.mark.parametrize("name", sorted(n for n, v in ENTRIES.items() if v[2] == "list_mx"))
def test_mx_list_entries_refuse_an_fp16x3_nerf_handle(name):
    e = _Entry(name)
    assert e(handles=e.make(PREC_FP16X3)) == ERR_UNSUPPORTED and e.named() and b"must be in fp16mx" in e.error(), e.error()


def test_mx_plane_entry_refuses_a_style_handle_without_streams():
    e = _Entry("tgtc_restyle_rays_trunk_folded_mx")
    assert e() == ERR_UNSUPPORTED and e.named() and b"no fp16mx streams" in e.error(), e.error()
    # the siblings on the same handle get past that point: the rule is the mx entry's alone
    for name in ("tgtc_restyle_rays_trunk", "tgtc_restyle_rays_trunk_folded"):
        assert _Entry(name)(R=0, count=0) == 0, name
