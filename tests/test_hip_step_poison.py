"""The decode step, every attention form, with everything it must not consume poisoned before every step.

Per case three runners on the same weights take the same tokens.  Before each step runner A gets the cache rows past its live
positions and the step's whole data scratch filled with a pattern (HipLlamaRunner.debug_poison, what = 1 | 2), runner B gets the same
fill with zeros, runner C is left alone.  A's logits must equal B's bit for bit at every position (the last step has no tail left),
and so must the live cache rows at the end; C must equal B (the hook changes nothing a step computes).  A kernel that multiplies a
dead row by a zero probability instead of masking it, takes a dead score into a maximum or a sum, or reads scratch that no launch of
the step wrote, gives NaN or another number under one of the patterns.

Each case names the form it is for; that the named form is what runs is asserted from debug_step_plan's words and the variant_of
rule (tests/poison.py), position by position.  The tap's attn_variant word takes the values 0, 1, 16 + 1 and 16 + 2 -- a plain 2 does
not exist: variant 2 is k_attn_flash's ticket form and only a flash context has one."""
import numpy as np
import pytest

from crabml_amd import synth
from tests.poison import (CACHE_TAIL, EXACT_ATTENTION, FLASH_TICKET, NO_PV_PRODUCER_WAVES, NO_STAGED_ATTENTION, PATTERNS, Q8K_ATTN_PRODUCER,
                          STEP_SCRATCH, ZERO, cache_rows, release_devices, same, same_cache, tokens_for, variant_of)  # noqa: F401 (autouse fixture)

pytestmark = pytest.mark.gpu

WHAT = CACHE_TAIL | STEP_SCRATCH


class Case:
    def __init__(self, form, shape, fmt, long_variant, seq=64, kv_f16=True, strict=False, graph=True, flags=0, long_from=8, words=None, mix=False,
                 tap_words=None):
        self.tap_words = tap_words or {}
        self.form, self.shape, self.fmt, self.long_variant, self.seq, self.kv_f16 = form, shape, fmt, long_variant, seq, kv_f16
        self.strict, self.graph, self.flags, self.long_from, self.words, self.mix = strict, graph, flags, long_from, words or {}, mix


STAGED, UNSTAGED = {"attn_s_rows": "> 0"}, {"attn_s_rows": 0}
# long_variant: what serves positions from `long_from` cached positions on (0: the context has no long form and stays on the short one)
CASES = [
    # one workgroup per head
    Case("k_attn<false>, f32 cache", "tiny-gqa", "Q4_0", 0, kv_f16=False, words={"attn_long_ok": 0, **UNSTAGED}),
    Case("k_attn<false>, f32 cache, seq_len 61", "tiny-gqa", "Q8_0", 0, seq=61, kv_f16=False, words={"attn_long_ok": 0, **UNSTAGED}),
    Case("k_attn<true> (NO_STAGED_ATTENTION)", "tiny-gqa", "Q4_0", 0, flags=NO_STAGED_ATTENTION, long_from=0, words=UNSTAGED),
    Case("k_attn_s", "tiny-gqa", "Q4_0", 0, long_from=0, words={"attn_s_rows": 64}),
    Case("k_attn_s, seq_len 61", "tiny-gqa", "Q8_0", 0, seq=61, long_from=0, words={"attn_s_rows": 61}),
    Case("k_attn_s + Q8_K producer, Q4_K body", "tiny-gqa", "Q4_K", 0, flags=Q8K_ATTN_PRODUCER, long_from=0,
         words={"attn_s_rows": 64, "q8k_producers": 1, "norm_epi_k": 1, "path": 2}, tap_words={"aq8": 1}),
    Case("k_attn_s, head_dim 48 (15m: no long form)", "15m", "Q4_0", 0, words={"attn_long_ok": 0, **STAGED}),
    # the exact long-context kernels
    Case("k_attn_scores / k_attn_softmax / k_attn_pv_split", "tiny-gqa", "Q4_0", 1, flags=EXACT_ATTENTION,
         words={"exact_long_ok": 1, "pv_split": 1, "attn_flash": 0, **STAGED}),
    Case("k_attn_scores / k_attn_softmax / k_attn_pv", "tiny-gqa", "Q4_0", 1, flags=EXACT_ATTENTION | NO_PV_PRODUCER_WAVES,
         words={"exact_long_ok": 1, "pv_split": 0, "attn_flash": 0}),
    Case("exact long, Q4_K body", "tiny-hd128", "Q4_K", 1, flags=EXACT_ATTENTION, words={"exact_long_ok": 1, "pv_split": 1, "path": 2}),
    # k_attn_flash
    Case("k_attn_flash, merge inside the launch below 768", "tiny-gqa", "Q4_0", 16 + 2, words={"attn_flash": 1, "flash_ticket": 0}),
    Case("k_attn_flash, seq_len 61", "tiny-gqa", "Q4_0", 16 + 2, seq=61, words={"attn_flash": 1, "exact_long_ok": 0}),
    Case("k_attn_flash, eager", "tiny-gqa", "Q8_0", 16 + 2, graph=False, words={"attn_flash": 1, "use_graph": 0}),
    Case("k_attn_flash, ticket form (FLASH_TICKET)", "tiny-gqa", "Q4_0", 16 + 1, flags=FLASH_TICKET, words={"attn_flash": 1, "flash_ticket": 1}),
    Case("k_attn_flash, Q4_1 body (Q8_1 planes)", "tiny-hd128", "Q4_1", 16 + 2, words={"attn_flash": 1}),
    Case("k_attn_flash, Q4_K_M body", "tiny-gqa", "Q4_K", 16 + 2, mix=True, words={"attn_flash": 1, "path": 2}),
    Case("k_attn_flash, head_dim 256 (tiny-gemma)", "tiny-gemma", "Q4_0", 16 + 2, words={"attn_flash": 1}),
    Case("k_attn_flash, group 7 (tiny-qwen2-g7)", "tiny-qwen2-g7", "Q4_0", 16 + 2, words={"attn_flash": 1}),
    # the strict-order device: the short form with sequential row sums, then the exact long-context kernels
    Case("strict device, short and long", "tiny-gqa", "Q4_0", 1, strict=True, words={"ordered": 1, "exact_long_ok": 1, "attn_flash": 0}),
    Case("strict device, Q4_K body, f32 cache", "tiny-gqa", "Q4_K", 0, strict=True, kv_f16=False, words={"ordered": 1, "attn_long_ok": 0, **UNSTAGED}),
]
# past 1024 cached positions, checked at positions 1029 .. 1032: k_attn_flash with its merge launch; the exact kernels, whose softmax
# row sum is a block tree there
LONG_CASES = [
    Case("k_attn_flash + k_attn_flash_merge past 768", "tiny-gqa", "Q4_0", 16 + 1, seq=1280, long_from=0, words={"attn_flash": 1}),
    Case("exact long, block-tree row sum past 1024", "tiny-gqa", "Q4_0", 1, seq=1280, long_from=0, flags=EXACT_ATTENTION,
         words={"exact_long_ok": 1, "attn_flash": 0}),
]


def make(ca, case, seed):
    model = synth.build_model(synth.SHAPES[case.shape], synth.TYPE_BY_NAME[case.fmt], seed=seed, k_m_mix=case.mix)
    dev = ca.HipTensorDevice(0, False, 0, case.strict)
    conf, w = synth.to_hip(model, dev)
    plan = ca.debug_step_plan(conf, w, dev, case.seq, case.kv_f16, case.graph, extra_flags=case.flags, attn_long_from=case.long_from)
    mk = lambda: ca.HipLlamaRunner(conf, w, dev, case.seq, case.kv_f16, case.graph, extra_flags=case.flags, attn_long_from=case.long_from)
    return model, plan, mk


def check_taps(case, plan, mk, toks, positions):
    """the same from the context itself: tapped steps of a spare runner report the attn_variant the rule gives (the fast device's
    fused steps; the strict-order device has no tap)"""
    if case.strict:
        return
    r = mk()
    for pos in range(max(positions) + 1):
        if pos in positions:
            tp = r.debug_tap(toks[pos], pos, 0)["plan"]
            assert tp["attn_variant"] == variant_of(plan, pos), (case.form, pos, tp)
            for word, want in case.tap_words.items():
                assert tp[word] == want, (case.form, pos, word, tp)
        else:
            r.forward_async(toks[pos], pos)


def check_plan(case, plan, positions):
    """the named form is what runs: the plan words the case states, and variant_of at every position"""
    for word, want in case.words.items():
        assert (plan[word] > 0) if want == "> 0" else (plan[word] == want), (case.form, word, plan)
    long_from = plan["attn_long_from"]
    for pos in positions:
        want = case.long_variant if case.long_variant and pos + 1 >= long_from else 0
        assert variant_of(plan, pos) == want, (case.form, pos, plan)
    print(f"{case.form}: {case.shape} {case.fmt}{'_M' if case.mix else ''} seq_len {case.seq} -> path {plan['path']} ordered {plan['ordered']}, "
          f"attn_variant {sorted({variant_of(plan, p) for p in positions})} from {long_from} cached positions, attn_s_rows {plan['attn_s_rows']}, "
          f"pv_split {plan['pv_split']}, flash_ticket {plan['flash_ticket']}, graph {plan['use_graph']}")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.form)
def test_poisoned_tail_and_scratch_change_no_step(ca, case):
    model, plan, mk = make(ca, case, seed=61)
    s, seq = model.shape, case.seq
    check_plan(case, plan, range(seq))
    if case.long_variant:
        assert 1 < plan["attn_long_from"] < seq  # the case runs its short form first, then the named one
    toks = tokens_for(s, seq)
    check_taps(case, plan, mk, toks, {0, min(plan["attn_long_from"], seq) - 1, seq - 1})

    def run(fill):
        r = mk()
        out = []
        for pos, t in enumerate(toks):
            if fill is not None:
                r.debug_poison(WHAT, *fill)
            out.append(r.forward(t, pos).copy())
        return out, cache_rows(r, s, case.kv_f16, seq, seq)

    base, base_cache = run(ZERO)
    assert all(np.all(np.isfinite(x)) for x in base), case.form
    plain, plain_cache = run(None)
    for pos in range(seq):
        assert same(plain[pos], base[pos]), f"{case.form}: the hook itself moved step {pos}"
    assert same_cache(plain_cache, base_cache), f"{case.form}: the hook itself moved the cache"
    for name, fill in PATTERNS.items():
        got, got_cache = run(fill)
        for pos in range(seq):
            assert same(got[pos], base[pos]), f"{case.form}: pattern {name} reached the logits of step {pos} (attn_variant {variant_of(plan, pos)})"
        assert same_cache(got_cache, base_cache), f"{case.form}: pattern {name} reached the live cache rows"


@pytest.mark.parametrize("case", LONG_CASES, ids=lambda c: c.form)
def test_poisoned_tail_and_scratch_past_1024_positions(ca, case):
    model, plan, mk = make(ca, case, seed=62)
    s, seq, first, last = model.shape, case.seq, 1029, 1032
    check_plan(case, plan, range(first, last + 1))
    toks = tokens_for(s, last + 1)
    check_taps(case, plan, mk, toks, {first, last})

    def run(fill):
        r = mk()
        for pos in range(first):
            r.forward_async(toks[pos], pos)
        out = []
        for pos in range(first, last + 1):
            if fill is not None:
                r.debug_poison(WHAT, *fill)
            out.append(r.forward(toks[pos], pos).copy())
        return out, cache_rows(r, s, case.kv_f16, last + 1, seq)

    base, base_cache = run(ZERO)
    assert all(np.all(np.isfinite(x)) for x in base), case.form
    plain, plain_cache = run(None)
    assert all(same(a, b) for a, b in zip(plain, base)) and same_cache(plain_cache, base_cache), f"{case.form}: the hook itself moved a step"
    for name, fill in PATTERNS.items():
        got, got_cache = run(fill)
        for i, (a, b) in enumerate(zip(got, base)):
            assert same(a, b), f"{case.form}: pattern {name} reached the logits of step {first + i}"
        assert same_cache(got_cache, base_cache), f"{case.form}: pattern {name} reached the live cache rows"


def test_the_hook_refuses_what_it_does_not_serve(ca):
    model = synth.build_model(synth.SHAPES["tiny-gqa"], synth.Q4_0, seed=63)
    dev = ca.HipTensorDevice(0)
    conf, w = synth.to_hip(model, dev)
    r = ca.HipLlamaRunner(conf, w, dev, 64, True)
    with pytest.raises(ca.CrabmlError):
        r.debug_poison(8, 0, 0)  # no such class
