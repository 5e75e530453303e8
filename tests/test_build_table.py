"""The build's one table of the companion libraries (companions.py) and its staleness check: the table names every library that
has a version script, the loaders follow from it, a compiler's .d file is read as make writes it, and after a build the .d files
name exactly the #include "..." closure of every source."""
import glob
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-inertial-odometry_amd", "csrc")
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def source_of(key):
    return g.COMPANIONS[key].get("source", "vio_%s.hip" % key)


def test_table_names_every_library_with_a_version_script():
    maps = glob.glob(os.path.join(CSRC, "libvio_*_hip.map"))
    assert sorted(g.COMPANIONS) == sorted(re.match(r"libvio_(\w+)_hip\.map$", os.path.basename(m)).group(1) for m in maps)
    assert len(g.COMPANIONS) == 17
    for key in g.COMPANIONS:
        assert os.path.exists(os.path.join(CSRC, source_of(key))), key


@pytest.mark.parametrize("key", sorted(g.COMPANIONS))
def test_loader_path_and_class_follow_from_the_table(vio, key):
    assert vio.COMPANIONS == g.COMPANIONS
    load = getattr(vio, "load_" + key)
    assert callable(load) and load.__name__ == "load_" + key
    assert load.__doc__ == "Load the %s (csrc/libvio_%s_hip.so)." % (g.COMPANIONS[key]["what"], key)
    assert getattr(vio, key.upper() + "_LIB") == os.path.join(CSRC, "libvio_%s_hip.so" % key)
    module, cls = g.COMPANIONS[key]["binding"].split(".")
    assert getattr(vio, cls) is getattr(getattr(vio, module), cls)
    assert getattr(vio, cls).__name__ == cls


def test_d_file_is_read_as_make_writes_it(tmp_path):
    root = tmp_path / "tree"
    base = root / "pkg" / "csrc"
    d = tmp_path / "x.d"
    d.write_text("diag/x.o: x.hip a.h \\\n  ../../include/b.h \\\n"
                 "  /usr/include/math.h with\\ space.h \\\n  %s/pkg/abs.h ../../../outside.h\n" % root)
    assert g.read_deps(str(d), str(base), str(root)) == [
        str(base / "x.hip"), str(base / "a.h"), str(root / "include" / "b.h"), str(base / "with space.h"), str(root / "pkg" / "abs.h")]
    # (a tree whose name only begins like the root's is outside it)
    d.write_text("x.o: %s-other/a.h\n" % root)
    assert g.read_deps(str(d), str(base), str(root)) == []


@pytest.fixture
def target(tmp_path):
    """target, its .d file, the two files that names, and a link-step dependency: all up to date."""
    for name, t in (("src.hip", 100), ("inc.h", 200), ("link.map", 250), ("t.d", 300), ("t.o", 300)):
        (tmp_path / name).write_text("t.o: src.hip \\\n inc.h /usr/include/math.h\n" if name == "t.d" else "")
        os.utime(tmp_path / name, (t, t))

    def stale():
        return g._stale(str(tmp_path / "t.o"), [str(tmp_path / "t.d")], [str(tmp_path / "link.map")], base=str(tmp_path), root=str(tmp_path))
    return tmp_path, stale


def test_up_to_date_target_is_not_stale(target):
    tmp, stale = target
    assert not stale()
    os.utime(tmp / "inc.h", (300, 300))         # as old as the target: not newer
    assert not stale()


@pytest.mark.parametrize("gone", ["t.o", "t.d", "inc.h", "src.hip", "link.map"])
def test_stale_when_a_file_is_missing(target, gone):
    tmp, stale = target
    os.remove(tmp / gone)
    assert stale()


@pytest.mark.parametrize("newer", ["inc.h", "src.hip", "link.map"])
def test_stale_when_a_listed_file_is_newer(target, newer):
    tmp, stale = target
    os.utime(tmp / newer, (301, 301))
    assert stale()


INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)


def include_closure(src):
    """`src` and every file it reaches through #include "...", each looked for beside the including file, in csrc/ and in include/."""
    seen, todo = set(), [os.path.join(CSRC, src)]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        for name in INCLUDE.findall(open(f).read()):
            found = [p for p in (os.path.normpath(os.path.join(d, name)) for d in (os.path.dirname(f), CSRC, os.path.join(ROOT, "include")))
                     if os.path.exists(p)]
            assert found, "%s includes %s, which is nowhere" % (f, name)
            todo.append(found[0])
    return seen


@pytest.mark.parametrize("src", sorted(source_of(k) for k in g.COMPANIONS) + g.HIP_SOURCES)
def test_d_file_names_the_include_closure(src):
    d = os.path.join(CSRC, os.path.splitext(src)[0] + ".d")
    assert os.path.exists(d), "build first: %s" % d
    assert set(g.read_deps(d, CSRC)) == include_closure(src)
