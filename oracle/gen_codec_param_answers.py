"""Writes tests/golden/codec_param_known_answers.json from the reference codec itself (oracle/_ref/libvkref.so):

    python oracle/gen_codec_param_answers.py

The cases (tests/codec_params.KNOWN_CASES) lie outside tolerance 0 .. 12 and max_epochs 0 .. 5; the file holds recorded
results only: per case the token count and the FNV-1a-64 of the stream(s) and of levelCut()."""
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


@contextlib.contextmanager
def quiet():
    """the reference prints its timings and statistics on stdout (file descriptor 1)"""
    sys.stdout.flush()
    keep, null = os.dup(1), os.open(os.devnull, os.O_WRONLY)
    os.dup2(null, 1)
    try:
        yield
    finally:
        os.dup2(keep, 1)
        os.close(keep)
        os.close(null)


def main():
    from oracle import oracle as O
    import codec_params as P
    O.build()
    assert O.ref_available(), "oracle/_ref/libvkref.so is not built (no reference sources at %s)" % O.ref_dir()
    cases = []
    for name, seed, shape, tol, ep, vname in P.KNOWN_CASES:
        with quiet():
            r = O.RefTree(P.volume(name, shape, seed), tolerance=tol, max_epochs=ep, midrange=vname == "mid").build()
        cases.append(P.known_record(O, r, name, seed, shape, tol, ep, vname))
    with open(P.KNOWN_ANSWERS, "w") as f:
        f.write('{"source": "RefTree, oracle/gen_codec_param_answers.py", "cases": [\n')
        f.write(",\n".join(json.dumps(c) for c in cases))
        f.write("\n]}\n")
    print("%d cases -> %s" % (len(cases), os.path.relpath(P.KNOWN_ANSWERS, ROOT)))


if __name__ == "__main__":
    main()
