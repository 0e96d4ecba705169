"""The adapter's stand-in interface is pinned to the reference's real one.

tests/adapter/harness.cpp re-declares IModelComponent / message_data by hand because the
reference's headers need Boost.  Every `virtual` declaration of the reference's
inst/include/imodel_component.hpp:60-172 (and of IVisitable, its base) and every message_data
constructor of inst/include/message_data.hpp:31-46 were parsed out of those headers, whitespace-
normalised, and recorded in tests/golden/reference_interface.json as SHA-256 digests (the
virtuals' names in clear): the stand-in must declare exactly those, token for token -- if it
drifts, this fails.  `python tests/test_adapter_interface_pin.py <reference checkout>` records
them again from a reference tree."""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIN = os.path.join(ROOT, "tests", "golden", "reference_interface.json")
HARNESS = os.path.join(ROOT, "tests", "adapter", "harness.cpp")


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def norm(text):
    """whitespace-insensitive token string"""
    text = re.sub(r"\s+", " ", text).strip()
    return re.sub(r"\s*([(),&*=;{}:])\s*", r"\1", text)


def class_body(text, name):
    m = re.search(r"\b(?:class|struct)\s+%s\b[^;{]*\{" % name, text)
    assert m, name
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[m.end():i - 1]


def virtual_signatures(body):
    """every `virtual ...` declaration up to its `;` or inline body, minus `inline` and the body"""
    out = []
    for m in re.finditer(r"\bvirtual\b[^;{]*", body):
        sig = m.group(0).replace("inline", " ")
        out.append(norm(sig))
    return out


def harness_text():
    return norm(strip_comments(open(os.path.join(ROOT, "tests", "adapter", "harness.cpp")).read()))


def digest(sig):
    return hashlib.sha256(sig.encode()).hexdigest()


def ctor_signatures(body):
    return [norm(m.group(0)) for m in re.finditer(r"\bmessage_data\s*\([^)]*\)", body)]


def record(ref_root):
    """The pin of the reference tree at ref_root (its inst/include headers) -> dict."""
    inc = os.path.join(ref_root, "inst", "include")
    ref = strip_comments(open(os.path.join(inc, "imodel_component.hpp")).read())
    vis = strip_comments(open(os.path.join(inc, "ivisitable.hpp")).read())
    sigs = virtual_signatures(class_body(ref, "IModelComponent")) + \
        [s for s in virtual_signatures(class_body(vis, "IVisitable")) if "~" not in s]
    sigs = [s for s in sigs if "~IModelComponent" not in s]
    msg = class_body(strip_comments(open(os.path.join(inc, "message_data.hpp")).read()), "message_data")
    base = re.search(r"\bclass\s+IModelComponent\s*:\s*public\s+(\w+)", ref)
    return {"source": "inst/include/{imodel_component,ivisitable,message_data}.hpp of the reference "
                      "(v3.5.0), whitespace-normalised by this module",
            "imodel_component_base": base.group(1) if base else None,
            "imodel_component_virtuals_sha256": sorted(digest(s) for s in sigs),
            "imodel_component_virtual_names": sorted(set(re.findall(
                r"\bvirtual\s+[\w:<> ]+?[ &*](\w+)\s*\(", class_body(ref, "IModelComponent")))),
            "message_data_constructors_sha256": sorted(digest(c) for c in ctor_signatures(msg))}


def pin():
    return json.load(open(PIN))


def harness_body(name):
    return class_body(strip_comments(open(HARNESS).read()), name)


def test_every_virtual_of_the_reference_interface_is_in_the_stand_in():
    p = pin()
    sigs = p["imodel_component_virtuals_sha256"]
    # the reference's interface as of v3.5.0: ten virtuals + accept (a new one must be adapted too)
    assert len(sigs) == 11, sigs
    have = harness_text()
    stand_in = norm(harness_body("IModelComponent"))
    mine = {digest(s): s for s in virtual_signatures(harness_body("IModelComponent")) if "~" not in s}
    for s in sigs:
        assert s in mine, "the reference declares a virtual (sha256 %s) tests/adapter/harness.cpp does not" % s
    # ... and the stand-in declares nothing the reference does not (destructor aside)
    for d, s in mine.items():
        assert d in sigs, "stand-in only: " + s
    # private getData: the adapter's override must sit behind `private:` like the reference's
    assert re.search(r"private:virtual unitval getData\(", stand_in)
    assert p["imodel_component_base"] == "IVisitable"
    assert have


def test_message_data_constructors_match_the_reference():
    ctors = pin()["message_data_constructors_sha256"]
    assert len(ctors) == 5, ctors
    mine = {digest(c) for c in ctor_signatures(harness_body("message_data"))}
    for c in ctors:
        assert c in mine, "the reference constructs a message_data (sha256 %s) the stand-in does not" % c


def test_the_product_adapter_overrides_exactly_those_virtuals():
    """include/hector_amd_component.hpp marks each of them `override` (so a drift of the base is a
    compile error in a host that builds against the real header)."""
    hdr = strip_comments(open(os.path.join(ROOT, "include", "hector_amd_component.hpp")).read())
    names = set(pin()["imodel_component_virtual_names"])
    names |= {"accept"}
    names -= {"run_spinup"}   # has a default body in the reference; the adapter keeps it
    for n in sorted(names):
        assert re.search(r"\b%s\s*\([^;{]*\)\s*(const\s*)?override" % n, hdr), n


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: %s <reference checkout>" % sys.argv[0])
    with open(PIN, "w") as f:
        json.dump(record(sys.argv[1]), f, indent=1)
        f.write("\n")
    print("wrote", PIN)
