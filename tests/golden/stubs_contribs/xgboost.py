"""The xgboost stand-in of tests/golden/stubs plus ``Booster.get_dump`` -- used ONLY by
make_golden_contribs.py, ahead of tests/golden/stubs on PYTHONPATH.

``get_dump()`` of a gblinear booster is one string, ``bias:\\n%g\\nweight:\\n%g\\n%g...``
(xgboost 0.7 ``GBLinearModel::DumpModel``); predict_by_cluster_rsat.py:106-108 parses it.
"""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    "_xgboost_base_stub", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "stubs", "xgboost.py"))
_base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_base)

DMatrix = _base.DMatrix


class Booster(_base.Booster):
    def get_dump(self):
        lines = ["bias:", "%g" % float(self.bias), "weight:"] + ["%g" % float(x) for x in self.w]
        return ["\n".join(lines) + "\n"]
