"""Generates tests/golden/ros_interfaces.json: the field declarations (type, name, order -- what the ROS md5sum is computed from;
comments dropped) of the reference's msg/LoopEdge.msg and srv/WholeImageDescriptorCompute.srv, so that
tests/test_ros_adapter_surface.py compares the shipped interface files with the reference's without a reference checkout.
Run: python tests/golden/make_ros_interfaces.py <reference checkout>"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
from test_ros_adapter_surface import INTERFACES, fields  # noqa: E402


def main():
    ref = Path(sys.argv[1])
    out = {"what": "field declarations (type, name) in file order of the reference's ROS interface files; '---' separates a "
                   "service's request from its response (tests/golden/make_ros_interfaces.py)"}
    for name in INTERFACES:
        out[name] = fields(ref / name)
    (HERE / "ros_interfaces.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
