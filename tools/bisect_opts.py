#!/usr/bin/env python3
"""which implementation switches make a flow deviate from the plain path?  A front end to tests/optmatrix.py (the covering array of every pair of switches).

usage: tools/bisect_opts.py FAMILY                 every pair row of the family against the PLAIN handle; the first row that deviates is shrunk
       tools/bisect_opts.py FAMILY name=value ...  that row (switches not named: at their defaults) against PLAIN, shrunk if it deviates
       tools/bisect_opts.py --rows FAMILY          print the rows (no GPU)
FAMILY: box ragged periodic moving exit circle2d.  Never on a row that ended in a GPU fault or a hang."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import optmatrix as om


def main(argv):
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 2
    list_rows = argv[0] == "--rows"
    args = argv[1:] if list_rows else argv
    if not args or args[0] not in om.FAMILIES or (list_rows and len(args) != 1):
        print(__doc__)
        return 2
    family = args[0]
    if list_rows:
        for i, r in enumerate(om.pair_rows(family)):
            print(i, {n: v for n, v in r.items() if v != om.FACTORS[n][0]}, "live:", sorted(om.live(r, family)))
        return 0
    if len(args) > 1:
        row = om.defaults(om.names(family))
        given = dict(a.split("=", 1) for a in args[1:] if "=" in a)
        if len(given) != len(args) - 1 or not set(given) <= set(row):
            print(__doc__)
            return 2
        row.update({k: int(v) for k, v in given.items()})
        return 0 if om.shrink(family, row) == {} else 1
    import waterlily_jl_amd as w
    w.core.device()
    try:
        ref, _, err = om.run(family, w, {n: om.PLAIN[n] for n in om.names(family)})
        assert err is None, err
        for i, row in enumerate(om.pair_rows(family)):
            w.lib().wl_reset_process_options()
            snaps, cnt, err = om.run(family, w, row)
            d = om.first_diff(snaps, ref) if err is None else None
            faults = om.counter_faults(row, family, cnt)
            print("row %2d %s %s" % (i, "error: " + err if err else ("differs: %r" % (d[:3],) if d else "same bits"), "; ".join(faults)))
            if err:
                return 1
            if d:
                om.shrink(family, row, w)
                return 1
    finally:
        w.lib().wl_reset_process_options()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
