"""One in-tree HIP library that is a unit of its own (libbeacon_actor.so, libbeacon_learner.so): built with hipcc on first use with
the flags of the main library (build.FLAGS) plus per-file flags, bound through ctypes in a table of its own.  The sidecar .sig holds
a hash of its sources, every header they include and the flags: staleness is decided by content, as for the main library
(build.py).  Concurrent builders are serialised by a file lock and build into a per-process object directory; the library and its
.sig are replaced atomically.  Stated once here; actor.py and learner.py each hold one Unit."""
import ctypes as C
import fcntl
import glob
import hashlib
import os
import shutil
import subprocess

from . import build as _build


class Unit(object):
    def __init__(self, name, file_flags, signatures, extra_deps=()):
        """`name`: "actor" -> csrc/actor/*.hip, include/beacon_actor.h, libbeacon_actor.so; `file_flags`: basename -> extra flags;
        `signatures`: symbol -> (restype, argtypes), every symbol the header declares; `extra_deps`: what the units include from
        outside their directory and their header."""
        self.name = name
        self.src_dir = os.path.join(_build.CSRC, name)
        self.header = os.path.join(_build.INC, "beacon_%s.h" % name)
        self.libname = "libbeacon_%s.so" % name
        self.lib = os.path.join(_build.PKG, self.libname)
        self.obj = os.path.join(_build.OBJ, name)
        self.file_flags, self.signatures, self.extra_deps = file_flags, signatures, list(extra_deps)
        self._loaded = None

    def sources(self):
        return sorted(glob.glob(os.path.join(self.src_dir, "*.hip")))

    def deps(self):
        return self.sources() + glob.glob(os.path.join(self.src_dir, "*.h")) + self.extra_deps + [self.header]

    def signature(self):
        h = hashlib.sha256()
        h.update(repr((_build.ARCH, _build.FLAGS, sorted(self.file_flags.items()))).encode())
        for f in sorted(self.deps()):
            h.update(os.path.basename(f).encode())
            with open(f, "rb") as fh:
                h.update(fh.read())
        return h.hexdigest()

    def stale(self):
        if not os.path.exists(self.lib) or not os.path.exists(self.lib + ".sig"):
            return True
        with open(self.lib + ".sig") as fh:
            return fh.read().strip() != self.signature()

    def build(self, force=False, verbose=False):
        """Compile csrc/<name>/*.hip for gfx950 and link the library.  Returns its path."""
        if not force and not self.stale():
            return self.lib
        cc = _build.hipcc()
        if cc is None:
            raise RuntimeError("hipcc not found: cannot build %s" % self.libname)
        with open(self.lib + ".lock", "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)               # one builder at a time per checkout
            try:
                if not force and not self.stale():         # another process built it while we waited
                    return self.lib
                sig = self.signature()
                objdir = os.path.join(self.obj, "p%d" % os.getpid())
                os.makedirs(objdir, exist_ok=True)
                objs = []
                for src in self.sources():
                    obj = os.path.join(objdir, os.path.basename(src)[:-4] + ".o")
                    cmd = [cc] + _build.FLAGS + self.file_flags.get(os.path.basename(src), []) + ["-I", _build.INC, "-c", src, "-o", obj]
                    if verbose:
                        print(" ".join(cmd), flush=True)
                    subprocess.check_call(cmd)
                    objs.append(obj)
                tmp = "%s.tmp%d" % (self.lib, os.getpid())
                cmd = [cc, "-shared", "-fPIC", "--offload-arch=" + _build.ARCH, "-o", tmp] + objs
                if verbose:
                    print(" ".join(cmd), flush=True)
                subprocess.check_call(cmd)
                os.replace(tmp, self.lib)
                with open(self.lib + ".sig.tmp", "w") as fh:
                    fh.write(sig + "\n")
                os.replace(self.lib + ".sig.tmp", self.lib + ".sig")
                shutil.rmtree(objdir, ignore_errors=True)
            finally:
                fcntl.flock(lock, fcntl.LOCK_UN)
        return self.lib

    def load(self):
        """dlopen the in-tree library (building it first when stale and hipcc is present); a missing library is an error."""
        if self._loaded is not None:
            return self._loaded
        path = self.lib
        if self.stale():
            if os.environ.get("BEACON_NO_BUILD") == "1":
                raise RuntimeError("%s is missing or stale and BEACON_NO_BUILD=1: run "
                                   "`python -c 'import __graft_entry__ as g; g.build()'` first" % self.libname)
            path = self.build()
        L = C.CDLL(path)
        for name, (res, args) in self.signatures.items():
            fn = getattr(L, name)                          # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        self._loaded = L
        return L
