"""Child process of test_intake.py: insert_raw under an environment that is read when the handle is created (BRISK_INTAKE_PIECE),
against insert_reads of the fragments' strings.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import brisk_amd as B  # noqa: E402
from intake_reference import fragment_strings, quality_case  # noqa: E402


def main():
    geo = tuple(int(v) for v in sys.argv[1:4])
    seqs, quals = quality_case(600, 13)
    rule = B.intake_rule(min_qual=20)
    frags, want = B.fragments_from_reads(seqs, quals, geo[0], rule)
    with B.BriskHip(*geo) as raw, B.BriskHip(*geo) as ref:
        got = raw.insert_raw(seqs, quals, rule)
        ref.insert_reads(fragment_strings(seqs, frags))
        equal = raw.checksum() == ref.checksum()
        table, st2 = raw.intake(seqs, quals, rule)  # the fragment table across pieces: read indices are the call's
        equal = equal and bool((table == frags).all()) and st2 == want
    print(json.dumps({"equal": bool(equal), "stats_equal": got == want, "n_short": want["n_short"], "n_bases_in": want["n_bases_in"],
                      "piece": os.environ.get("BRISK_INTAKE_PIECE")}))


if __name__ == "__main__":
    main()
