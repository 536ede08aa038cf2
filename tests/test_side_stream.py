"""CPU-only: the context's auxiliary stream is reached through FmkSide (finmlkit_amd/csrc/fmk_common.h, fmk_api.hip) alone.

Outside those two files no source redirects the context's stream by assigning to it, names the auxiliary stream or its events, or
parks the allocator's frees by hand: each of these is one half of a fork / join that the helper writes once, with the error paths."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "finmlkit_amd", "csrc")
ALLOWED = ("fmk_common.h", "fmk_api.hip")
FORBIDDEN = {
    "assignment to the context's stream": re.compile(r"\bctx->stream\s*=(?!=)"),
    "an event of the auxiliary stream by index": re.compile(r"\baev\s*\["),
    "the auxiliary stream or one of its events by name": re.compile(r"->\s*aux(_fork|_done|_landed)?\b"),
    "fmk_pool_defer": re.compile(r"\bfmk_pool_defer\s*\("),
    "fmk_ctx_aux": re.compile(r"\bfmk_ctx_aux\s*\("),
}


def hand_made_forks(files):
    bad = []
    for fn, txt in files:
        if fn in ALLOWED:
            continue
        for no, line in enumerate(txt.splitlines(), 1):
            for what, rx in FORBIDDEN.items():
                if rx.search(line):
                    bad.append(f"{fn}:{no}: {what}: {line.strip()}")
    return bad


def _sources():
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".h", ".cpp")):
            yield fn, open(os.path.join(CSRC, fn), errors="replace").read()


def test_auxiliary_stream_only_through_the_helper():
    bad = hand_made_forks(_sources())
    assert not bad, "hand-made fork / join on the auxiliary stream (use FmkSide):\n" + "\n".join(bad)


def test_guard_catches_each_pattern():
    for line in ["        ctx->stream = ctx->aux;",
                 "        ctx->stream = keep;",
                 "        FMK_HIP(ctx, hipEventRecord(ctx->aev[0], ctx->stream));",
                 "            hipError_t e = hipEventRecord(ctx->aev[3], side);",
                 "        (void)hipStreamSynchronize(c->aux);",
                 "        FMK_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->aux_done, 0));",
                 "        (void)fmk_pool_defer(ctx, 1);",
                 "    if (d_median && nb >= 4096 && fmk_ctx_aux(ctx) == FMK_OK) {"]:
        assert hand_made_forks([("fmk_barflow.hip", line)]), line
        assert not hand_made_forks([("fmk_api.hip", line)]), line
    for line in ["    if (ctx->stream == other) return FMK_OK;",
                 "    k_bar_dir<false><<<(unsigned)blocks, 256, 0, ctx->stream>>>(d_price);",
                 "        FMK_TRY(side.fork(true));",
                 "                hipStream_t st = (k > 0 && forked) ? side.stream() : nullptr;"]:
        assert not hand_made_forks([("fmk_barflow.hip", line)]), line


def test_the_helper_refuses_nesting_and_scratch_on_the_side():
    """the two rules nobody can break silently any more: one fork per context at a time, no context scratch on the auxiliary stream"""
    api = open(os.path.join(CSRC, "fmk_api.hip")).read()
    fork = api[api.index("int FmkSide::fork("):]
    fork = fork[:fork.index("\n}\n")]
    assert re.search(r"if \(ctx->side_open\) return fmk_set_error\(", fork)
    scratch = api[api.index("int fmk_scratch("):]
    scratch = scratch[:scratch.index("\n}\n")]
    assert re.search(r"if \(ctx->aux && ctx->stream == ctx->aux\)\s*(//[^\n]*)?\n\s*return fmk_set_error\(", scratch)
