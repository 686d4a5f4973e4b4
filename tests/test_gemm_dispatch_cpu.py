"""The host side of the bf16 GEMM without a GPU (csrc/gemm.hip: check, plan, run).

vds_gemm_plan runs the argument check and the planning function of vds_gemm_bf16 / vds_gemm_bf16_grouped and launches
nothing, so the tile choice -- tiling, grid, K split, atomics, tile order, narrow last column, where the column sums are
taken -- is pinned here against tests/golden/gemm_plans.json: the decisions of the dispatcher BEFORE it was split into
check / plan / run, recorded once from a build of that commit (profiles/gemm_dispatch/verdict.txt says how).  The refusal
rows run through vds_gemm_bf16, vds_gemm_bf16_grouped and vds_gemm_plan, which must agree: every call here is refused by
a host-side check, nothing is launched or read.

VDS_LIB_PATH=<a build without vds_gemm_plan> runs the refusal rows alone (the plan rows are skipped there and only there).
"""
import ctypes as C
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_census as G  # noqa: E402

from video_diffusion_speedrun_amd import _lib  # noqa: E402

NT, NN, TN = _lib.VDS_NT, _lib.VDS_NN, _lib.VDS_TN
STORE, GELU, GATE, DGELU, F32 = _lib.EPI_STORE, _lib.EPI_BIAS_GELU, _lib.EPI_GATE_RES, _lib.EPI_DGELU, _lib.EPI_F32
LAYOUTS = {"NT": NT, "NN": NN, "TN": TN}
EPILOGUES = {"STORE": STORE, "BIAS_GELU": GELU, "GATE_RES": GATE, "DGELU": DGELU, "F32": F32}
PAIRS = (("NT", "STORE"), ("NT", "BIAS_GELU"), ("NT", "GATE_RES"), ("NN", "STORE"), ("NN", "DGELU"), ("TN", "F32"))
TILES = (0, 128, 256, 2)
FIELDS = [n for n, _ in _lib.GemmPlanInfo._fields_]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plans.json")
ERR_ARG, ERR_UNSUPPORTED = -1, -2
P = 0x10000   # a non-null, 16-byte aligned address: nothing below is launched or read


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def has_plan():
    return hasattr(C.CDLL(_lib.LIB_PATH), "vds_gemm_plan")


def args(layout, epi, M, N, K, split_k=1, colsum=False, rpb=0, **over):
    """a call that passes every check when (layout, epi) is a pair of the table: dense operands, every pointer its epilogue
    uses set; `over` replaces fields"""
    lay, e = LAYOUTS[layout], EPILOGUES[epi]
    a = _lib.GemmArgs(lay, e, M, N, K, P, M if lay == TN else K, P, K if lay == NT else N, P, N, None, 0, None, None, 0,
                      None, 0, rpb, split_k, P if colsum else None)
    if e in (GELU, GATE):
        a.C2, a.ldc2 = P, N
    if e in (GATE, DGELU):
        a.aux, a.ldaux = P, N
    if e == GATE:
        a.gate, a.ldgate = P, N
    for k, v in over.items():
        setattr(a, k, v)
    return a


# ---- the plan table -----------------------------------------------------------------------------------------------------
def case(layout, epi, M, N, K, split_k=1, colsum=False, groups=None, tile=0, det=False, knobs=None):
    """groups = (lead, period, L): the grouped entry with rows_per_batch = L"""
    name = f"{layout}-{epi}-{M}x{N}x{K}-s{split_k}-t{tile}"
    name += ("-colsum" if colsum else "") + (f"-g{groups[0]}.{groups[1]}.{groups[2]}" if groups else "")
    name += ("-det" if det else "") + "".join(f"-{k}={v:g}" for k, v in sorted((knobs or {}).items()))
    return dict(id=name, layout=layout, epi=epi, M=M, N=N, K=K, split_k=split_k, colsum=colsum, groups=groups, tile=tile,
                det=det, knobs=knobs or {})


def plan_cases():
    out = []
    # the GEMMs of the C3b / C5 train step at per-GPU batch 12 (tools/bench_gemm_tiles.py and the model): 8192 + 16 token
    # rows per sample, D = 1152, context [512, 4096], patches of 16 x 2 x 2 x 2 values, 8 token frames
    Mt, Mp, D = 12 * 8208, 12 * 8192, 1152
    linears = (("qkv", Mt, 3 * D, D), ("proj", Mt, D, D), ("fc1", Mt, 4 * D, D), ("fc2", Mt, D, 4 * D),
               ("ctxkv", 12 * 512, 2 * D, 4096), ("patch", Mp, D, 128), ("final", Mt, 128, D), ("final", Mp, 128, D))
    for name, M, N, K in linears:
        out.append(case("NT", "BIAS_GELU" if name == "fc1" else "STORE", M, N, K))
        out.append(case("NN", "STORE", M, K, N))                       # dx = dy W
        for s in (0, -1):
            out.append(case("TN", "F32", N, K, M, split_k=s))         # dW = dy^T x, the library's own split
        if name in ("proj", "fc2"):
            out.append(case("NT", "GATE_RES", M, N, K))
            out.append(case("NT", "GATE_RES", M, N, K, groups=(16, 8, 8208)))
    # the census shapes under every forced tiling; TN with every form of split_k (tile 2 + explicit split: the mid TN path)
    for tile in TILES:
        for M, N, K in G.SHAPES_NT:
            out.append(case("NT", "STORE", M, N, K, tile=tile))
            out.append(case("NN", "STORE", M, N, K, tile=tile))
        for M, N, K in G.SHAPES_TN:
            for s in (0, -1, 1, 3, -3):
                out.append(case("TN", "F32", M, N, K, split_k=s, tile=tile))
        for M, N, K in G.SHAPES_GROUPED:   # a grouped GATE_RES call in each tiling
            g = G.GROUPED
            out.append(case("NT", "GATE_RES", M, N, K, groups=(g["lead"], g["period"], G.ROWS_PER_BATCH), tile=tile))
        out.append(case("NT", "GATE_RES", Mt, D, D, groups=(16, 8, 8208), tile=tile))
        for s in (0, -1, 1, 3, -3):
            out.append(case("TN", "F32", 3 * D, D, Mt, split_k=s, tile=tile))
        # K below 128 (no 256 x 128, no 256^2 by the model), K in 128 .. 255 (no 256^2 by the model)
        for K in (64, 120, 128, 192, 248, 256):
            out.append(case("NT", "STORE", Mt, D, K, tile=tile))
            out.append(case("NN", "STORE", Mt, 4 * D, K, tile=tile))
        # N % 256 in 0, 72, 128, 136: the narrow last column on and off
        for N in (1024, 1096, 1152, 1160):
            out.append(case("NT", "STORE", Mt, N, D, tile=tile))
            out.append(case("NT", "STORE", Mt, N, D, tile=tile, knobs={"gemm_narrow": 0}))
        # NN + DGELU with column sums: where the model takes 256^2 (fused), 128^2 (small), and under each forced tiling; in
        # deterministic mode the sums are a pass of their own in every tiling
        for M, N, K in ((Mt, 4 * D, D), (264, 328, 328), (6144, 384, 1152)):
            for det in (False, True):
                out.append(case("NN", "DGELU", M, N, K, colsum=True, tile=tile, det=det))
                out.append(case("NN", "DGELU", M, N, K, tile=tile, det=det))
    # With gemm_mid_factor at its default (1.3) no NT / NN shape makes the model choose 256 x 128 (a scan of every M <= 102400,
    # N <= 5120 in full tiles finds none: a round of it never undercuts both other tilings); priced at 1.0 it does
    for det in (False, True):
        out.append(case("NN", "DGELU", Mt, D, 4 * D, colsum=True, det=det, knobs={"gemm_mid_factor": 1.0}))
    out.append(case("NT", "STORE", Mt, D, D, knobs={"gemm_mid_factor": 1.0}))
    # the auto split: shapes that take 128^2 and 256 x 128; the joint_xcd group clamped to 1 and to tiles_m; gemm_tn_joint off
    for M, N, K in ((128, 1152, Mp), (384, 384, Mt), (512, 4096, 512), (3 * D, D, Mt), (2 * D, 4096, 6144),
                    (512, 17408, 512), (4 * D, 128, Mt)):
        for s in (0, -1):
            out.append(case("TN", "F32", M, N, K, split_k=s))
            out.append(case("TN", "F32", M, N, K, split_k=s, det=True))
        out.append(case("TN", "F32", M, N, K, split_k=0, knobs={"gemm_tn_joint": 0}))
    return list({c["id"]: c for c in out}.values())   # (the lists overlap in a few shapes: one row each)


def run_plan(lib, c, ws):
    """the plan of one case as a list in FIELDS order (or the refusal code); `ws`: the address of 4096 aligned bytes.
    Knobs, forced tile and mode are put back."""
    prev = {k: lib.vds_knob_get(k.encode()) for k in c["knobs"]}
    try:
        for k, v in c["knobs"].items():
            assert lib.vds_knob_set(k.encode(), float(v)) == 0
        assert lib.vds_gemm_force_tile(c["tile"]) >= 0
        if c["det"]:
            assert lib.vds_set_deterministic(1, ws, 4096) >= 0
        g = c["groups"]
        a = args(c["layout"], c["epi"], c["M"], c["N"], c["K"], c["split_k"], c["colsum"], rpb=g[2] if g else 0)
        info = _lib.GemmPlanInfo()
        rc = lib.vds_gemm_plan(C.byref(a), C.byref(_lib.ModGroups(g[0], g[1])) if g else None, C.byref(info))
        return [getattr(info, f) for f in FIELDS] if rc == 0 else rc
    finally:
        lib.vds_set_deterministic(0, None, 0)
        lib.vds_gemm_force_tile(0)
        for k, v in prev.items():
            lib.vds_knob_set(k.encode(), v)


def test_plan_equals_the_recorded_decisions_of_the_old_dispatcher(lib):
    if not has_plan():
        pytest.skip("a build without vds_gemm_plan (the refusal rows alone are run against it)")
    golden = json.load(open(GOLDEN))
    assert golden["fields"] == FIELDS
    cases = plan_cases()
    assert sorted(golden["plans"]) == sorted(c["id"] for c in cases)
    buf = C.create_string_buffer(4096 + 16)   # deterministic mode wants a 16-byte aligned workspace; never touched
    ws = (C.addressof(buf) + 15) & ~15
    wrong = {}
    for c in cases:
        got = run_plan(lib, c, ws)
        if got != golden["plans"][c["id"]]:
            wrong[c["id"]] = (got, golden["plans"][c["id"]])
    assert not wrong, (len(wrong), list(wrong.items())[:5])
    assert lib.vds_knob_get(b"deterministic") == 0.0 and lib.vds_gemm_force_tile(0) == 0


def test_plan_table_reaches_every_branch():
    """what the issue of the refactor asks the shape list to reach, read off the recorded table itself"""
    golden = json.load(open(GOLDEN))["plans"]
    rows = [(c, dict(zip(FIELDS, golden[c["id"]]))) for c in plan_cases()]
    default = [(c, p) for c, p in rows if not c["knobs"] and c["tile"] == 0]

    def some(pred, among=rows):
        return any(pred(c, p) for c, p in among)

    for layout in LAYOUTS:
        for tile in TILES:
            assert some(lambda c, p: c["layout"] == layout and c["tile"] == tile)
    for tiling in (128, 2, 256):
        assert some(lambda c, p: c["groups"] and p["tiling"] == tiling)
        assert some(lambda c, p: c["colsum"] and c["tile"] == tiling and p["tiling"] == tiling and p["colsum"] == 2)
    assert some(lambda c, p: c["colsum"] and p["tiling"] == 256 and p["colsum"] == 1, default)           # fused by the model
    assert some(lambda c, p: c["colsum"] and c["det"] and p["tiling"] == 256 and p["colsum"] == 2)       # trailing on 256^2
    assert some(lambda c, p: c["colsum"] and c["tile"] == 0 and p["tiling"] == 2)                         # the model's 256x128
    assert some(lambda c, p: c["layout"] == "TN" and c["tile"] == 2 and c["split_k"] == 3 and p["tiling"] == 2
                and p["split_k"] == 3)                                                                    # the mid TN path
    assert some(lambda c, p: c["layout"] == "TN" and c["split_k"] == -3 and p["atomic"] == 1 and p["split_k"] == 3)
    for tiling in (128, 2):
        assert some(lambda c, p: c["split_k"] == 0 and p["tiling"] == tiling and p["split_k"] > 1, default)
    assert some(lambda c, p: c["split_k"] == 0 and p["split_k"] == 1 and p["atomic"] == 0, default)
    assert some(lambda c, p: c["split_k"] == -1 and p["split_k"] == 1 and p["atomic"] == 1, default)
    # the joint_xcd group: clamped to 1 with more than one tile row, clamped to tiles_m, and unclamped
    auto2 = [(c, p) for c, p in default if c["split_k"] == 0 and p["tiling"] == 2 and p["joint_xcd"]]
    assert some(lambda c, p: p["group_m"] == 1 and p["tiles_m"] > 1 and p["tiles_m"] * p["split_k"] < 4, auto2)
    assert some(lambda c, p: p["group_m"] == p["tiles_m"] > 1, auto2)
    assert some(lambda c, p: 1 < p["group_m"] < p["tiles_m"], auto2)
    assert some(lambda c, p: c["knobs"].get("gemm_tn_joint") == 0 and p["joint_xcd"] == 0 and p["group_m"] == 2)
    for rem, narrow in ((0, 0), (72, 1), (128, 1), (136, 0)):
        assert some(lambda c, p: c["N"] % 256 == rem and p["tiling"] == 256 and p["narrow"] == narrow, default)
    assert some(lambda c, p: c["knobs"].get("gemm_narrow") == 0 and c["N"] % 256 == 72 and p["tiling"] == 256
                and p["narrow"] == 0)
    assert some(lambda c, p: c["K"] < 128 and c["layout"] != "TN")
    assert some(lambda c, p: 128 <= c["K"] < 256 and c["layout"] != "TN")
    assert not some(lambda c, p: c["K"] < 128 and c["tile"] == 0 and p["tiling"] != 128 and c["layout"] != "TN")


# ---- refusals -----------------------------------------------------------------------------------------------------------
def refusal_rows():
    """(what, args, groups or None, code).  Rows without groups go through vds_gemm_bf16 and vds_gemm_bf16_grouped(NULL)."""
    rows = []
    L = 73
    gate = dict(M=2 * L, N=64, K=64, rpb=L)
    grp = (16, 3)
    # the grouped misfits
    rows += [
        ("groups with NN", args("NN", "STORE", 2 * L, 64, 64, rpb=L), grp, ERR_ARG),
        ("groups with TN + F32", args("TN", "F32", 64, 64, 64, rpb=8), grp, ERR_ARG),
        ("groups with NT + STORE", args("NT", "STORE", 2 * L, 64, 64, rpb=L), grp, ERR_ARG),
        ("groups with NT + BIAS_GELU", args("NT", "BIAS_GELU", 2 * L, 64, 64, rpb=L), grp, ERR_ARG),
        ("groups with a pair outside the table", args("NN", "GATE_RES", 2 * L, 64, 64, rpb=L), grp, ERR_ARG),
        ("groups without rows_per_batch", args("NT", "GATE_RES", 2 * L, 64, 64), grp, ERR_ARG),
        ("lead < 0", args("NT", "GATE_RES", **gate), (-1, 2), ERR_ARG),
        ("period < 1", args("NT", "GATE_RES", **gate), (16, 0), ERR_ARG),
        ("lead > L", args("NT", "GATE_RES", **gate), (L + 1, 1), ERR_ARG),
        ("(L - lead) % period", args("NT", "GATE_RES", **gate), (16, 4), ERR_ARG),
        ("M % L", args("NT", "GATE_RES", 2 * L + 1, 64, 64, rpb=L), grp, ERR_ARG),
    ]
    # colsum needs DGELU and C
    for layout, epi in PAIRS:
        if epi != "DGELU":
            rows.append((f"colsum with {layout} + {epi}", args(layout, epi, 64, 64, 64, colsum=True), None, ERR_ARG))
    rows.append(("colsum with C == NULL", args("NN", "DGELU", 64, 64, 64, colsum=True, C=None), None, ERR_ARG))
    # an operand of 4 GiB: ((rows - 1) * ld + cols) * 2 bytes >= 2^32 from R + 1 rows of 2^15 elements on
    R = 1 << 16
    rows += [
        ("A of 4 GiB (NT)", args("NT", "STORE", R + 1, 64, 64, lda=1 << 15), None, ERR_UNSUPPORTED),
        ("B of 4 GiB (NT)", args("NT", "STORE", 64, R + 8, 64, ldb=1 << 15), None, ERR_UNSUPPORTED),
        ("B of 4 GiB (NN)", args("NN", "STORE", 64, 64, R + 8, lda=1 << 17, ldb=1 << 15), None, ERR_UNSUPPORTED),
        ("A of 4 GiB (TN)", args("TN", "F32", 64, 64, R + 1, lda=1 << 15), None, ERR_UNSUPPORTED),
        ("A one row short of 4 GiB (NT): refused for ldc instead", args("NT", "STORE", R, 64, 64, lda=1 << 15, ldc=68), None,
         ERR_ARG),
        ("4 GiB and a pair outside the table", args("NT", "DGELU", R + 1, 64, 64, lda=1 << 15), None, ERR_UNSUPPORTED),
        ("4 GiB and C == NULL: the operand test comes first", args("NT", "STORE", R + 1, 64, 64, lda=1 << 15, C=None), None,
         ERR_UNSUPPORTED),
    ]
    # VDS_ERR_ARG wins over a pair outside the table
    rows += [
        ("pair outside the table and ldc % 8", args("NT", "DGELU", 64, 64, 64, ldc=68), None, ERR_ARG),
        ("pair outside the table and a split", args("NN", "F32", 64, 64, 64, split_k=2), None, ERR_ARG),
        ("pair outside the table and C == NULL", args("NN", "GATE_RES", 64, 64, 64, C=None, C2=None), None, ERR_ARG),
        ("epilogue 64 is not a public value", args("NT", "STORE", 64, 64, 64, epilogue=64), None, ERR_UNSUPPORTED),
        ("epilogue -1", args("NT", "STORE", 64, 64, 64, epilogue=-1), None, ERR_UNSUPPORTED),
    ]
    return rows


def outside_rows():
    """every (layout, epilogue) pair outside the table, with and without colsum (DGELU: the only epilogue that may carry
    one), at a shape every tiling takes"""
    rows = []
    for layout in LAYOUTS:
        for epi in EPILOGUES:
            if (layout, epi) in PAIRS:
                continue
            for colsum in ((False, True) if epi == "DGELU" else (False,)):
                M, N, K = 512, 512, 512
                rows.append((f"{layout} + {epi}" + (" + colsum" if colsum else ""), args(layout, epi, M, N, K, colsum=colsum)))
    assert len(rows) == 3 * 5 - 6 + 2
    return rows


def call_all(lib, a, groups):
    """the codes of the entries that take these arguments: vds_gemm_bf16 (groups None), _grouped, vds_gemm_plan"""
    g = C.byref(_lib.ModGroups(*groups)) if groups else None
    codes = [lib.vds_gemm_bf16_grouped(C.byref(a), g, None)]
    if groups is None:
        codes.append(lib.vds_gemm_bf16(C.byref(a), None))
    if has_plan():
        codes.append(lib.vds_gemm_plan(C.byref(a), g, C.byref(_lib.GemmPlanInfo())))
    return codes


@pytest.mark.parametrize("row", refusal_rows(), ids=lambda r: r[0])
def test_refusals(lib, row):
    what, a, groups, code = row
    codes = call_all(lib, a, groups)
    assert set(codes) == {code}, (what, codes)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("row", outside_rows(), ids=lambda r: r[0])
def test_pair_outside_the_table_is_unsupported_in_every_tiling(lib, row, tile):
    what, a = row
    try:
        assert lib.vds_gemm_force_tile(tile) >= 0
        assert set(call_all(lib, a, None)) == {ERR_UNSUPPORTED}, (what, tile, call_all(lib, a, None))
    finally:
        lib.vds_gemm_force_tile(0)


def test_plan_entry_checks_its_own_argument(lib):
    if not has_plan():
        pytest.skip("a build without vds_gemm_plan")
    assert lib.vds_gemm_plan(C.byref(args("NT", "STORE", 64, 64, 64)), None, None) == ERR_ARG
    info = _lib.GemmPlanInfo(tiling=-7)
    assert lib.vds_gemm_plan(C.byref(args("NT", "DGELU", 64, 64, 64)), None, C.byref(info)) == ERR_UNSUPPORTED
    assert info.tiling == -7   # left alone on a refusal
