"""Host-side check of the form decision (form_decision of csrc/catre_forms.h, exported as catre_form_decision): which kernel
form, row split, run length and grid a launch of an encoder stage takes.

The reference is `_Ladders`: the if / else-if ladders the launches carried BEFORE the decision became one function
(launch_stn3d / launch_stnkd / launch_trunk, the pre-checks of the two screen probes, the three catre_train_*_fwd entries
and the bf16 pair gate), mirrored line by line from that source together with the helper predicates they were built from.
It reads the RAW 13-bit switch state (ids 0 - 9 of catre_form_switch, bits 10 - 12 the env-only STN arms), like that code did.

The decision is compared with it for every switch state: all 8192 at one shape per caller, and for every shape, forced run
length and CU count over every combination of the bits that caller's ladder reads (the rest held at their defaults - the
8192-state sweep shows that they do not matter)."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

from catre_amd import hip

TP = 64
(TRUNK4, STN4, STN_PAIR, ROTW, FC_TAIL, SCREEN, SCREEN_STN, SCREEN_POOL, SCREEN_RUN, SCREEN_F16, POOL_STN, RUN_STN,
 F16_STN) = range(13)
DEFAULTS = sum(1 << b for b in range(13) if b not in (ROTW, FC_TAIL))


def _rule(B, N, M, cus):
    """screen_run_rule, as in tests/test_screen_run_host.py"""
    TN, TM = (N + TP - 1) // TP, (M + TP - 1) // TP
    slots1 = -(-B * (TN + TM) // cus)
    for S in range(16, 1, -1):
        if -(-B * (-(-TN // S) + -(-TM // S)) // cus) * S <= slots1:
            return S
    return 1


def row_split(tiles):
    return 4 if tiles * 4 <= 256 else 2 if tiles * 2 <= 256 else 1


def row_split8(tiles):
    return 8 if tiles * 8 <= 256 else row_split(tiles)


def stn_pairs(B, N, M):
    return B * (((N + TP - 1) // TP + 1) // 2 + ((M + TP - 1) // TP + 1) // 2)


def stn_pair_runs(B, N, M, SP):
    return B * ((((N + TP - 1) // TP + 1) // 2 + SP - 1) // SP + (((M + TP - 1) // TP + 1) // 2 + SP - 1) // SP)


class _Ladders:
    """The launches' own gating before the decision function, one method per ladder."""

    def __init__(self, raw, cus, run_len, bf_pair_min):
        on = lambda b: bool(raw >> b & 1)
        self.trunk4_on, self.stn4_on, self.stn_pair_on = on(TRUNK4), on(STN4), on(STN_PAIR)
        self.screen_on = on(SCREEN)
        self.screen_stn_on = on(SCREEN) and on(SCREEN_STN)
        self.screen_pool_on = on(SCREEN_POOL)
        self.screen_run_on = on(SCREEN_POOL) and on(SCREEN_RUN)
        self.screen_pool_stn_on = self.screen_pool_on and on(POOL_STN)
        self.screen_run_stn_on = self.screen_run_on and self.screen_stn_on and self.screen_pool_stn_on and on(RUN_STN)
        self.screen_f16_on = on(SCREEN_POOL) and on(SCREEN_F16)
        self.screen_f16_stn_on = self.screen_f16_on and self.screen_pool_stn_on and on(F16_STN)
        self.cus, self.run_len, self.bf_pair_min = cus, run_len, bf_pair_min

    def screen_run_len(self, B, N, M):
        return self.run_len if self.run_len > 0 else _rule(B, N, M, self.cus)

    def stn_pair_form(self, tiles, B, N, M):
        return row_split8(tiles) == 1 and self.stn4_on and self.stn_pair_on and stn_pairs(B, N, M) >= 256

    def launch_stn(self, B, N, M, split, probe):                     # launch_stn3d and launch_stnkd: the same ladder
        tiles = B * ((N + TP - 1) // TP + (M + TP - 1) // TP)
        if split:
            return "split_rs", row_split(tiles), 1, tiles * row_split(tiles)
        S = self.screen_run_len(B, N, M) if self.stn_pair_form(tiles, B, N, M) and self.screen_run_stn_on and not probe else 1
        if S > 1:
            SP = S // 2
            return ("run_f16" if self.screen_f16_stn_on else "run"), 1, SP, stn_pair_runs(B, N, M, SP)
        if self.stn_pair_form(tiles, B, N, M) and (self.screen_stn_on or probe):
            f16 = self.screen_f16_stn_on
            return ("screen_f16" if f16 else "screen_pool" if self.screen_pool_stn_on else "screen"), 1, 1, stn_pairs(B, N, M)
        if self.stn_pair_form(tiles, B, N, M):
            return "pair", 1, 1, stn_pairs(B, N, M)
        if row_split8(tiles) == 1 and self.stn4_on:
            return "wave4", 1, 1, tiles
        return "rs8", row_split8(tiles), 1, tiles * row_split8(tiles)

    def launch_trunk(self, B, N, M, split, probe):
        tiles = B * ((N + TP - 1) // TP + (M + TP - 1) // TP)
        if split:
            return "split_rs", row_split(tiles), 1, tiles * row_split(tiles)
        full4 = row_split8(tiles) == 1 and self.trunk4_on
        S = self.screen_run_len(B, N, M) if full4 and self.screen_on and self.screen_run_on else 1
        if S > 1:
            runs = B * (((N + TP - 1) // TP + S - 1) // S + ((M + TP - 1) // TP + S - 1) // S)
            return ("run_f16" if self.screen_f16_on else "run"), 1, S, runs
        if full4 and (self.screen_on or probe):
            f16 = self.screen_f16_on
            return ("screen_f16" if f16 else "screen_pool" if self.screen_pool_on else "screen"), 1, 1, tiles
        if full4:
            return "wave4", 1, 1, tiles
        return "rs8", row_split8(tiles), 1, tiles * row_split8(tiles)

    def trunk_screen_probe(self, B, N, M):                           # catre_trunk_screen_probe
        tiles = B * ((N + TP - 1) // TP + (M + TP - 1) // TP)
        if row_split8(tiles) != 1 or not self.trunk4_on:
            return ("unsupported",)
        return self.launch_trunk(B, N, M, False, True)

    def stn_screen_probe(self, B, N, M):                             # catre_stn_screen_probe, either STN
        tiles = B * ((N + TP - 1) // TP + (M + TP - 1) // TP)
        if not self.stn_pair_form(tiles, B, N, M):
            return ("unsupported",)
        return self.launch_stn(B, N, M, False, True)

    def refine_iter_bf(self, B, N, M):                               # the three encoder launches of the bf16 / fp16 chain
        TN, TM = (N + TP - 1) // TP, (M + TP - 1) // TP
        pairs = B * ((TN + 1) // 2 + (TM + 1) // 2)
        return ("bf_pair", 1, 1, pairs) if pairs >= self.bf_pair_min else ("bf", 1, 1, B * (TN + TM))

    def train_stn_fwd(self, B, N, M, mode, rows):                    # catre_train_stn3d_fwd and catre_train_stnkd_fwd
        tiles = B * (N + M) // TP
        bf_pairs = stn_pairs(B, N, M)                                # (bf_pairs there: the same expression)
        if mode == "bf16" and bf_pairs >= self.bf_pair_min:
            return "train_bf_pair", 1, 1, bf_pairs
        if mode == "bf16":
            return "train_bf", 1, 1, tiles
        if mode == "split":
            return "train_split", 1, 1, tiles
        if not rows and self.stn4_on and self.stn_pair_on and stn_pairs(B, N, M) >= 256:
            return "train_pair", 1, 1, stn_pairs(B, N, M)
        return "train_rs1", 1, 1, tiles

    def train_trunk_fwd(self, B, N, M, mode):                        # catre_train_trunk_fwd
        tiles = B * (N + M) // TP
        if mode == "bf16":
            TN, TM = N // TP, M // TP
            return "train_bf_pair", 1, 1, B * ((TN + 1) // 2 + (TM + 1) // 2)
        if mode == "split":
            return "train_split", 1, 1, tiles
        if self.trunk4_on and row_split8(tiles) == 1:
            return "train_wave4", 1, 1, tiles
        return "train_rs1", 1, 1, tiles


# every caller: (name, stage, mode, save, rows, probe, the switch bits its ladder reads, the mirror)
STN_BITS = (STN4, STN_PAIR, SCREEN, SCREEN_STN, SCREEN_POOL, SCREEN_RUN, SCREEN_F16, POOL_STN, RUN_STN, F16_STN)
TRUNK_BITS = (TRUNK4, SCREEN, SCREEN_POOL, SCREEN_RUN, SCREEN_F16)
CALLERS = []
for _stage in ("stn3d", "stnkd"):
    CALLERS += [
        (_stage, "fp32", 0, 0, 0, STN_BITS, lambda L, B, N, M: L.launch_stn(B, N, M, False, False)),
        (_stage, "fp32", 0, 0, 1, STN_BITS, lambda L, B, N, M: L.stn_screen_probe(B, N, M)),
        (_stage, "split", 0, 0, 0, (), lambda L, B, N, M: L.launch_stn(B, N, M, True, False)),
        (_stage, "bf16", 0, 0, 0, (), lambda L, B, N, M: L.refine_iter_bf(B, N, M)),
        (_stage, "fp32", 1, 1, 0, (STN4, STN_PAIR), lambda L, B, N, M: L.train_stn_fwd(B, N, M, "fp32", True)),
        (_stage, "fp32", 1, 0, 0, (STN4, STN_PAIR), lambda L, B, N, M: L.train_stn_fwd(B, N, M, "fp32", False)),
        (_stage, "split", 1, 1, 0, (), lambda L, B, N, M: L.train_stn_fwd(B, N, M, "split", True)),
        (_stage, "bf16", 1, 1, 0, (), lambda L, B, N, M: L.train_stn_fwd(B, N, M, "bf16", True)),
    ]
CALLERS += [
    ("trunk", "fp32", 0, 0, 0, TRUNK_BITS, lambda L, B, N, M: L.launch_trunk(B, N, M, False, False)),
    ("trunk", "fp32", 0, 0, 1, TRUNK_BITS, lambda L, B, N, M: L.trunk_screen_probe(B, N, M)),
    ("trunk", "split", 0, 0, 0, (), lambda L, B, N, M: L.launch_trunk(B, N, M, True, False)),
    ("trunk", "bf16", 0, 0, 0, (), lambda L, B, N, M: L.refine_iter_bf(B, N, M)),
    ("trunk", "fp32", 1, 1, 0, (TRUNK4,), lambda L, B, N, M: L.train_trunk_fwd(B, N, M, "fp32")),
    ("trunk", "split", 1, 1, 0, (), lambda L, B, N, M: L.train_trunk_fwd(B, N, M, "split")),
    ("trunk", "bf16", 1, 1, 0, (), lambda L, B, N, M: L.train_trunk_fwd(B, N, M, "bf16")),
]

# (B, N, M) on each side of every threshold of the ladders; the training entries take those with N, M multiples of 64, M > 0
SHAPES = [
    (1, 1024, 1024), (2, 1024, 1024), (4, 1024, 1024), (5, 1024, 1024),   # row_split8 = 8, 4, 2 (128 tiles), 1 (160 tiles)
    (32, 100, 70), (33, 100, 70),                                          # 128 / 132 tiles: row_split8 2 / 1
    (64, 64, 64), (65, 64, 64),                                            # the same boundary on whole tiles (128 / 130 tiles)
    (51, 384, 256), (128, 64, 64),                                         # stn_pairs 255 / 256
    (255, 64, 0), (256, 64, 0),                                            # ... and on a single cloud per object
    (73, 448, 320), (256, 64, 64),                                         # bf16 pairs 511 / 512
    (64, 1024, 1024), (200, 1024, 1024), (256, 1024, 1024),                # the run rule: 8, 1, 16
    (64, 960, 448), (200, 960, 448), (200, 100, 70), (64, 100, 70),
]
RUN_LENS = (0, 1, 2, 16)
CUS = (256, 304, 64)
BF_MINS = (512, 0, 1 << 30)


def _decide():
    fn = hip.load().catre_form_decision
    out = (ctypes.c_int * 4)()

    def decide(stage, mode, save, rows, probe, B, N, M, raw, cus, run_len, bf_min):
        if fn(stage, mode, save, rows, probe, B, N, M, raw, cus, run_len, bf_min, out):
            return None
        return hip.KERNEL_FORMS[out[0]], out[1], out[2], out[3]
    return decide


def _check(decide, caller, raw, B, N, M, cus, run_len, bf_min):
    stage, mode, save, rows, probe, _, mirror = caller
    want = mirror(_Ladders(raw, cus, run_len, bf_min), B, N, M)
    got = decide(hip.STAGES[stage], hip.MODES[mode], save, rows, probe, B, N, M, raw, cus, run_len, bf_min)
    where = (stage, mode, save, rows, probe, B, N, M, bin(raw), cus, run_len, bf_min)
    assert got is not None, where
    if want[0] == "unsupported":                                           # the probes' CATRE_ERR_UNSUPPORTED
        assert got[0] == "unsupported", (where, got)
    else:
        assert got == want, (where, got, want)


def _shapes(caller):
    return [s for s in SHAPES if not caller[2] or (s[1] % TP == 0 and s[2] % TP == 0 and s[2] > 0)]


def test_every_switch_state_at_one_shape_per_caller():
    decide = _decide()
    for caller in CALLERS:
        for B, N, M in ((256, 1024, 1024), (128, 64, 64)):                  # every rung reachable; the pair threshold
            for raw in range(1 << 13):
                _check(decide, caller, raw, B, N, M, 256, 0, 512)


@pytest.mark.parametrize("stage", ["stn3d", "stnkd", "trunk"])
def test_every_shape_run_length_and_cu_count_over_the_bits_a_caller_reads(stage):
    decide = _decide()
    n = 0
    for caller in CALLERS:
        if caller[0] != stage:
            continue
        bits = caller[5]
        bf_mins = BF_MINS if caller[1] == "bf16" else (512,)
        runs = list(itertools.product(RUN_LENS, CUS)) if caller[1] == "fp32" and not caller[2] else [(0, 256)]
        for states in itertools.product((0, 1), repeat=len(bits)):
            raw = DEFAULTS
            for b, v in zip(bits, states):
                raw = raw | 1 << b if v else raw & ~(1 << b)
            for (B, N, M), (run_len, cus), bf_min in itertools.product(_shapes(caller), runs, bf_mins):
                _check(decide, caller, raw, B, N, M, cus, run_len, bf_min)
                n += 1
    assert n > 1000


def test_the_shapes_sit_on_both_sides_of_every_threshold():
    tiles = lambda B, N, M: B * ((N + TP - 1) // TP + (M + TP - 1) // TP)
    assert {row_split8(tiles(*s)) for s in SHAPES} == {8, 4, 2, 1}
    assert tiles(32, 100, 70) == tiles(64, 64, 64) == 128 and row_split8(129) == 1
    assert {stn_pairs(51, 384, 256), stn_pairs(128, 64, 64), stn_pairs(255, 64, 0), stn_pairs(256, 64, 0)} == {255, 256}
    assert stn_pairs(73, 448, 320) == 511 and stn_pairs(256, 64, 64) == 512
    assert [_rule(B, 1024, 1024, 256) for B in (64, 200, 256)] == [8, 1, 16]
    decide = _decide()
    seen = {decide(hip.STAGES[c[0]], hip.MODES[c[1]], c[2], c[3], c[4], B, N, M, raw, 256, 0, 512)[0]
            for c in CALLERS for B, N, M in _shapes(c) for raw in (DEFAULTS, DEFAULTS & ~(1 << SCREEN_F16), DEFAULTS & ~(1 << SCREEN_POOL),
                                                                   DEFAULTS & ~(1 << SCREEN), DEFAULTS & ~(1 << SCREEN_RUN), 0)}
    assert seen == set(hip.KERNEL_FORMS)                                   # every form is reached


def test_the_shapes_of_the_training_encoder_forward_test_take_the_forms_it_names():
    """The (mode, B, N, M) rows of tests/test_train_encoder_fwd.py, which checks the SAVE kernels form by form on the GPU
    and asserts these same decisions there: a threshold that moves fails here first, and names the GPU cases to re-shape."""
    form = lambda stage, mode, B, N, M, raw=DEFAULTS, rows=True: hip.form_decision(stage, mode, B, N, M, raw, save=True, rows=rows,
                                                                                  bf_pair_min=512)[0]
    all3 = lambda mode, B, N, M, raw=DEFAULTS, rows=True: tuple(form(s, mode, B, N, M, raw, rows or s == "trunk")
                                                                for s in ("stn3d", "stnkd", "trunk"))
    # fp32, rows saved: the smallest grids; 132 tiles, with and without the one-wave-per-SIMD trunk
    assert all3("fp32", 1, 64, 64) == all3("fp32", 2, 192, 64) == ("train_rs1",) * 3
    assert all3("fp32", 33, 128, 128) == ("train_rs1", "train_rs1", "train_wave4")
    assert all3("fp32", 33, 128, 128, raw=DEFAULTS & ~(1 << TRUNK4)) == ("train_rs1",) * 3
    # fp32, STN rows not saved: below the pair threshold, and 256 pairs of an odd tile count with and without `stn_pair`
    assert all3("fp32", 2, 192, 64, rows=False) == ("train_rs1",) * 3
    assert stn_pairs(64, 192, 192) == 256 and (192 // TP) % 2 == 1
    assert all3("fp32", 64, 192, 192, rows=False) == ("train_pair", "train_pair", "train_wave4")
    assert all3("fp32", 64, 192, 192, rows=False, raw=DEFAULTS & ~(1 << STN_PAIR)) == ("train_rs1", "train_rs1", "train_wave4")
    assert all3("fp32", 64, 192, 192) == ("train_rs1", "train_rs1", "train_wave4")
    assert all3("split", 2, 192, 64) == all3("split", 33, 128, 128) == ("train_split",) * 3
    # bf16: one-tile STN kernels next to the trunk's pair kernel; 512 pairs
    assert all3("bf16", 2, 192, 64) == ("train_bf", "train_bf", "train_bf_pair")
    assert stn_pairs(128, 192, 192) == 512 and all3("bf16", 128, 192, 192) == ("train_bf_pair",) * 3
    # the B = 3 batches its batch-independence cases run next to the large grids
    assert all3("bf16", 3, 192, 192) == ("train_bf", "train_bf", "train_bf_pair") and all3("fp32", 3, 128, 128) == ("train_rs1",) * 3


def test_nonsense_is_refused():
    decide = _decide()
    ok = (0, 0, 0, 0, 0, 4, 64, 64, DEFAULTS, 256, 0, 512)
    assert decide(*ok) is not None
    for i, bad in ((0, 3), (0, -1), (1, 3), (5, 0), (6, 0), (7, -1), (8, 1 << 13), (8, -1), (9, 0), (10, 17), (10, -1)):
        args = list(ok)
        args[i] = bad
        assert decide(*args) is None, args
    assert decide(0, 1, 0, 0, 1, 4, 64, 64, DEFAULTS, 256, 0, 512) is None    # a probe is fp32
    assert decide(0, 0, 1, 0, 1, 4, 64, 64, DEFAULTS, 256, 0, 512) is None    # ... and no training forward
    assert decide(0, 0, 0, 1, 0, 4, 64, 64, DEFAULTS, 256, 0, 512) is None    # rows without saves
    assert decide(0, 2, 1, 0, 0, 4, 64, 64, DEFAULTS, 256, 0, 512) is None    # only the fp32 backward recomputes its rows
    assert decide(2, 0, 1, 0, 0, 4, 64, 64, DEFAULTS, 256, 0, 512) is None    # ... and only the STNs'
    assert hip.load().catre_form_decision(*ok, None) == -1


def test_form_switch_sets_the_raw_bit_and_the_decision_ignores_a_refined_bit_while_its_base_is_off():
    """Two halves: catre_form_switch reads back the RAW bit (`screen_stn` set while `screen` is off reads as set), and the
    decision, handed such a switch word, takes the same form as with the refined bit off.  That the launches hand it this
    process's word (effective_forms(forms())) is what the GPU form-against-form tests show, not this one."""
    was = {n: hip.form_switch(n) for n in ("screen", "screen_stn")}
    try:
        hip.form_switch("screen", False)
        hip.form_switch("screen_stn", True)
        assert hip.form_switch("screen_stn") is True and hip.form_switch("screen") is False     # the raw bit reads back
        hip.form_switch("screen_stn", False)
        assert hip.form_switch("screen_stn") is False
        assert hip.load().catre_form_switch(10, -1) == -1 and hip.load().catre_form_switch(-1, -1) == -1  # the arms: env only
    finally:
        for n, v in was.items():
            hip.form_switch(n, v)
    off = DEFAULTS & ~(1 << SCREEN)                                                              # an explicit switch word
    for stage in ("stn3d", "stnkd"):
        a = hip.form_decision(stage, "fp32", 256, 1024, 1024, off)
        b = hip.form_decision(stage, "fp32", 256, 1024, 1024, off & ~(1 << SCREEN_STN))
        assert a == b == ("pair", 1, 1, 256 * 16)
        assert hip.form_decision(stage, "fp32", 256, 1024, 1024, DEFAULTS)[0] == "run_f16"


def test_host_code_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/host/forms_san.cpp, a stand-alone program, drives the switch table, the decision and the bundle builders of
    csrc/catre_forms.h (no HIP in there) in a -fsanitize=address,undefined build of its own.  The sanitizer runtimes are
    linked statically, so the program runs in whatever environment the suite runs in."""
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler: g++, clang++ or the ROCm toolchain's clang++"
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else ["-static-libsan"]
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "forms_san.cpp")
    exe = str(tmp_path / "forms_san")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                   + static + [src, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "forms_san ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
