"""Generates tests/golden/model_xml.json: the elements and attributes of the reference model file (jitterbug_dmc/jitterbug.xml) that
tests/test_model.py::test_spec_matches_reference_xml compares model_spec.SPEC with, so that the test runs without the reference.

Kept: compiler, option, default/geom, the worldbody bodies `jitterbug` and `target` with their bodies / geoms / joints, actuator/general -
and of those only the attributes the test reads, as the strings the file holds (the test parses them as it parsed the XML).

    python tools/gen_golden_model_xml.py <path of the reference's jitterbug_dmc/jitterbug.xml>
"""
import json
import os
import sys
import xml.etree.ElementTree as ET

KEEP_ATTRS = ("name", "type", "size", "pos", "fromto", "density", "axis", "stiffness", "damping", "coordinate", "timestep",
              "gear", "ctrlrange", "gainprm", "biasprm", "biastype", "gaintype", "dyntype")
BODY_KIDS = ("body", "geom", "joint")


def node(el, kids=()):
    return {"tag": el.tag, "attrib": {k: v for k, v in el.attrib.items() if k in KEEP_ATTRS},
            "children": [body(c) if c.tag == "body" else node(c) for c in el if c.tag in kids]}


def body(el):
    return node(el, BODY_KIDS)


def extract(root):
    out = []
    for c in root:
        if c.tag in ("compiler", "option"):
            out.append(node(c))
        elif c.tag == "default":
            out.append(node(c, ("geom",)))
        elif c.tag == "worldbody":
            wb = node(c)
            wb["children"] = [body(b) for b in c.findall("body") if b.attrib.get("name") in ("jitterbug", "target")]
            out.append(wb)
        elif c.tag == "actuator":
            out.append(node(c, ("general",)))
    return {"tag": root.tag, "attrib": {}, "children": out}


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    tree = extract(ET.parse(sys.argv[1]).getroot())
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "model_xml.json")
    json.dump({"generator": "tools/gen_golden_model_xml.py", "source": "reference jitterbug_dmc/jitterbug.xml (elements and attributes test_model.py reads)",
               "tree": tree}, open(path, "w"), indent=1)
    print("wrote", path)
