"""Line coverage of the oracle under a given load, measured with gcov: an instrumented copy of oracle/ is built into a temporary
directory (never into oracle/), the load runs in a child process (the counters are written when it exits), and the
per-instantiation counts gcov reports for templates are folded into one count per source line.

    with Coverage() as cov:
        cov.run("from tests import contact_corpus as C; C.oracle_answers(C.corpus())")
        lines = cov.lines()          # {"mgf_collision.hpp": {line: count}, ...}; a line that is absent is not executable
        entered = cov.functions()    # {"mgf_geom.hpp": [(start, end, count), ...], ...}
"""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
# the oracle's own flags (oracle/Makefile) but for -O0 --coverage: the same f32 sequence, every line its own counter
FLAGS = ["-O0", "--coverage", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]


def available():
    return shutil.which("gcov") is not None and shutil.which("g++") is not None


class Coverage:
    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="mgf_oracle_cov_")
        self.lib = os.path.join(self.dir, "libmgf_oracle_cov.so")
        self._folded = None

    def __enter__(self):
        obj = os.path.join(self.dir, "oracle_capi.o")
        subprocess.check_call(["g++"] + FLAGS + ["-c", os.path.join(ORACLE, "oracle_capi.cpp"), "-o", obj], cwd=self.dir)
        subprocess.check_call(["g++", "--coverage", "-shared", "-o", self.lib, obj], cwd=self.dir)
        return self

    def __exit__(self, *exc):
        shutil.rmtree(self.dir, ignore_errors=True)

    def reset(self):
        """forget the counts gathered so far (a second measurement with the same build)"""
        for f in os.listdir(self.dir):
            if f.endswith(".gcda"):
                os.unlink(os.path.join(self.dir, f))
        self._folded = None

    def run(self, code):
        """run `code` in a child interpreter whose oracle binding loads the instrumented library"""
        env = dict(os.environ, MGF_ORACLE_LIB=self.lib, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=env)
        self._folded = None

    def _fold(self):
        if self._folded is None:
            subprocess.check_call(["gcov", "--json-format", "oracle_capi.gcda"], cwd=self.dir, stdout=subprocess.DEVNULL)
            with gzip.open(os.path.join(self.dir, "oracle_capi.gcov.json.gz"), "rt") as f:
                doc = json.load(f)
            lines, funcs = {}, {}
            for fl in doc["files"]:
                name = os.path.basename(fl["file"])
                if not os.path.exists(os.path.join(ORACLE, name)):
                    continue
                per = lines.setdefault(name, {})
                for ln in fl["lines"]:   # one record per (line, instantiation)
                    per[ln["line_number"]] = per.get(ln["line_number"], 0) + ln["count"]
                ranges = {}
                for fn in fl["functions"]:
                    key = (fn["start_line"], fn["end_line"])
                    ranges[key] = ranges.get(key, 0) + fn["execution_count"]
                funcs[name] = sorted((s, e, c) for (s, e), c in ranges.items())
            self._folded = (lines, funcs)
        return self._folded

    def lines(self):
        return self._fold()[0]

    def functions(self):
        return self._fold()[1]
