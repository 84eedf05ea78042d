"""The device mailbox (csrc/mailbox.hpp: dk::Mail, dk_ctx::d_mail / h_mail) is addressed by member name only.  A bare word number in one of its
users would bring back what the struct removed: two stages sharing a word unnoticed, and copy lengths nobody can check against what is read."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "dark_amd", "csrc")
BARE = (
    r"mail\s*\[\s*[0-9]",                # mail[12] inside a kernel
    r"_mail\s*\+\s*[0-9]",               # ctx->d_mail + 980
    r"h_mail\s*\[",                      # ctx->h_mail[989], ctx->h_mail[16 + s]: the mailbox is a struct, not an array
    r"hipMem(?:cpy|set)Async\([^;]*_mail[^;]*[,(]\s*[0-9]+\s*\*\s*sizeof",  # a copy or fill of it that counts words by hand
)


def test_no_bare_word_numbers_address_the_mailbox():
    sources = [p for p in glob.glob(os.path.join(CSRC, "*")) if os.path.basename(p) != "mailbox.hpp"]
    assert len(sources) > 10 and os.path.exists(os.path.join(CSRC, "mailbox.hpp"))
    hits = []
    for path in sources:
        with open(path, encoding="utf-8", errors="replace") as f:
            text = f.read()
        for pattern in BARE:
            hits += ["%s: %s" % (os.path.basename(path), m.group(0)) for m in re.finditer(pattern, text)]
    assert not hits, hits


def test_context_allocates_the_struct():
    with open(os.path.join(CSRC, "abi.cpp"), encoding="utf-8") as f:
        abi = f.read()
    assert abi.count("sizeof(dk::Mail)") == 3 and not re.search(r"_mail[^;]*1024", abi)  # device, pinned host, the clear
