"""The suite rebuilds libawry_hip.so only when build.stale() says so: every file the sources include, directly or through
another header, has to be one that stale() looks at -- else an edited kernel header leaves the suite testing the old
library."""
import os
import re

import pytest

from awry_amd import build

INCLUDE = re.compile(r'^\s*#\s*include\s*"([^"]+)"', re.M)


def included_files():
    """-> {normalised path: the file that first included it} over the #include "..." graph of build.SOURCES"""
    seen, todo = {}, [os.path.join(build.CSRC, f) for f in build.SOURCES]
    while todo:
        src = todo.pop()
        with open(src, encoding="utf-8", errors="replace") as f:
            text = f.read()
        for name in INCLUDE.findall(text):
            p = os.path.normpath(os.path.join(os.path.dirname(src), name))
            if p not in seen:
                seen[p] = src
                todo.append(p)
    return seen


def test_every_included_header_is_watched():
    watched = {os.path.normpath(os.path.join(build.CSRC, f)) for f in build.HEADERS}
    reached = included_files()
    assert len(reached) >= 10  # (the walk itself works: awry_hip.hip alone reaches the kernel headers)
    for p, by in sorted(reached.items()):
        assert os.path.isfile(p), "%s includes %s, which does not exist" % (by, p)
        assert p in watched, "%s (included by %s) is not in build.HEADERS: editing it would not rebuild the library" % (p, os.path.basename(by))
    for f in build.SOURCES + build.HEADERS:
        assert os.path.isfile(os.path.join(build.CSRC, f)), f


@pytest.mark.parametrize("name", ["lcx.hip.h", "lcx_kernels.hip.h", "kernels.hip.h", "kernels_nt2_kmer.hip.h", "count_plan.h", os.path.join("..", "..", "include", "awry_hip.h")])
def test_stale_sees_an_edited_header(monkeypatch, name):
    """stale() itself: with only `name` newer than the library, the library is stale; with nothing newer, it is not"""
    target = os.path.normpath(os.path.join(build.CSRC, name))
    assert target in included_files()
    newer = {"on": True}
    so = os.path.normpath(build.SO)
    exists = os.path.exists

    def mtime(p):
        p = os.path.normpath(p)
        if p == so:
            return 100.0
        return 200.0 if newer["on"] and p == target else 50.0

    monkeypatch.setattr(build.os.path, "exists", lambda p: os.path.normpath(p) == so or exists(p))
    monkeypatch.setattr(build.os.path, "getmtime", mtime)
    assert build.stale()
    newer["on"] = False
    assert not build.stale()
