"""build.py lists its translation units and headers by name (tools/build_trace.sh globs): a .hip file missing from SOURCES is not
linked, and a header missing from HEADERS is not hashed, so an edit to it leaves a stale library that still passes the check."""
import os
import re

from buzzdetect_amd import build


def _hip_files():
    return sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))


def test_sources_are_the_hip_files_of_csrc():
    assert len(set(build.SOURCES)) == len(build.SOURCES)
    assert set(build.SOURCES) == set(_hip_files())
    assert set(build.FILE_FLAGS) <= set(build.SOURCES)


def test_every_included_project_header_is_hashed():
    hashed = {os.path.normpath(os.path.join(build.CSRC, h)) for h in build.HEADERS}
    todo = [os.path.join(build.CSRC, f) for f in _hip_files()]
    seen = set()
    while todo:                                   # the .hip files and, through them, the headers' own includes
        path = todo.pop()
        if path in seen:
            continue
        seen.add(path)
        with open(path) as f:
            names = re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M)
        for name in names:
            inc = os.path.normpath(os.path.join(os.path.dirname(path), name))
            assert os.path.exists(inc), f"{path} includes {name}, which is not there"
            assert inc in hashed, f"{os.path.relpath(path, build.CSRC)} includes {name}, which build.HEADERS does not list"
            todo.append(inc)
    assert {p for p in seen if not p.endswith(".hip")} == hashed, "build.HEADERS lists a header nothing includes"
