"""Child process of the crafted-field tests: encodes the named cases of tests/field_cases.py with one library and prints a JSON
object name -> digest of (packets, stats).  usage: field_worker.py ref|hip NAME...   (hip: under whatever environment the
parent set, DSV2_SIDE_FORCE_FALLBACK for one)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import field_cases as F  # noqa: E402


def main(argv):
    which, names = argv[0], argv[1:]
    if which == "ref":
        lib = F.load_field_ref()
        setter = F.ref_setter(lib)
    else:
        import dsvabi as A
        from hipabi import bind
        lib = bind(A.load_hip())
        setter = F.hip_setter(lib)
    out = {}
    for name in names:
        out[name] = F.digest(*F.encode_case(lib, setter, F.BY_NAME[name]))
    if which == "hip":
        out["side_flag_count"] = lib.dsv2hip_enc_side_flag_count()
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
