"""CPU-only: the context mailbox (fmk_mail, finmlkit_amd/csrc/fmk_common.h) is reached through its named fields alone.

Outside the layout header and the context's create / destroy, `d_mail` / `h_mail` may only be followed by `->`: a slot number,
pointer arithmetic or a cast of the bare pointer would bring back the shared, untyped slots the named layout replaced."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "finmlkit_amd", "csrc")
BARE = re.compile(r"\b[dh]_mail\b(?!->)")


def _allowed(fn, line):
    if fn == "fmk_common.h":
        return True
    if fn == "fmk_api.hip":      # create / destroy: allocation, clearing and release of the two copies
        return re.search(r"hipHostMalloc|hipMalloc|memset\(c->h_mail, 0, sizeof\(fmk_mail\)\)|hipFree|hipHostFree", line) is not None
    return False


def bare_uses(files):
    bad = []
    for fn, txt in files:
        for no, line in enumerate(txt.splitlines(), 1):
            if BARE.search(line) and not _allowed(fn, line):
                bad.append(f"{fn}:{no}: {line.strip()}")
    return bad


def _sources():
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".h", ".cpp")):
            yield fn, open(os.path.join(CSRC, fn), errors="replace").read()


def test_mailbox_only_through_named_fields():
    bad = bare_uses(_sources())
    assert not bad, "raw mailbox slots (use a named field of fmk_mail):\n" + "\n".join(bad)


def test_guard_catches_raw_slots():
    for line in ["    int *d = (int *)(ctx->d_mail + 44);",
                 "    double *d_acc = (double *)ctx->d_mail;",
                 "    FMK_HIP(ctx, hipMemcpyAsync(ctx->h_mail, d_res, 16, hipMemcpyDeviceToHost, ctx->stream));",
                 "    const int64_t m = ctx->h_mail[0];"]:
        assert bare_uses([("fmk_volume.hip", line)]), line
    assert not bare_uses([("fmk_volume.hip", "    int *d_mis = &ctx->d_mail->vol.mismatch;")])
