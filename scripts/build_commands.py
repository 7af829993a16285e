"""Every command the in-tree build runs, normalised: what profiles/build_layer_identity.md compares between two checkouts.

    python scripts/build_commands.py OUT.txt [libraries] [plugins]      (from the root of the checkout it is to describe)

Runs every builder with force=True, verbose=True -- the main library, the actor, the learner, the torch extension, then
jit.prebuild(verbose=True), which compiles only the plugins that are not there yet: start from a tree without beacon_amd/_jit --
and collects the printed command lines.  The process id, the per-process object directory, the checkout's root and the compilers'
paths become placeholders; the list is sorted and written to OUT.txt; its sha256, the number of commands and the same hash with the
plugins' name suffix (the hash of their dependencies) masked are printed.  It uses public names only, so it runs in a checkout from
before build.py had one routine.  Default: both stages.  HIPCC may name a stand-in compiler for the `plugins` stage alone (one that
writes its -o file): the command lines do not depend on what the compiler does, and prebuild() needs only the main library to be
real."""
import contextlib
import hashlib
import io
import os
import re
import shutil
import sys

ROOT = os.getcwd()
sys.path.insert(0, ROOT)


def main():
    from beacon_amd import actor, build, jit, learner, torch_ext
    out, stages = io.StringIO(), sys.argv[2:] or ["libraries", "plugins"]
    with contextlib.redirect_stdout(out):
        if "libraries" in stages:
            build.build_lib(force=True, verbose=True)
            actor.build_actor(force=True, verbose=True)
            learner.build_learner(force=True, verbose=True)
            torch_ext.build_ext(force=True, verbose=True)
        plugins = [p for p in jit.prebuild(verbose=True) if p] if "plugins" in stages else []
    lines = []
    for l in out.getvalue().splitlines():
        cc, _, rest = l.partition(" ")
        name = "<HIPCC>" if cc == build.hipcc() else "<CXX>" if cc == (os.environ.get("CXX") or shutil.which("g++")) else None
        if name is None:
            continue                                   # (not a command line)
        rest = re.sub(r"\S*/_obj/(?:\w+/)?p\d+", "<OBJDIR>", rest).replace(ROOT, "<ROOT>")
        lines.append(name + " " + re.sub(r"\.tmp\d+", ".tmp<PID>", rest))
    lines.sort()
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
    masked = sorted(re.sub(r"_[0-9a-f]{12}\.so", "_<HASH>.so", l) for l in lines)
    for what, ls in (("as printed", lines), ("plugin hash suffix masked", masked)):
        print("%d commands, %d plugins, %s: sha256 %s" % (len(ls), len(plugins), what, hashlib.sha256("\n".join(ls).encode()).hexdigest()))


if __name__ == "__main__":
    main()
