"""The public Python surface of sdrgpu.filter and sdrgpu.fft does not move: for every public class,
its sorted public names, the signature of the class and of each public callable, and which names
are properties, against tests/golden/python_surface.json.  The golden file is written from the
package as it was before a change (`python tests/test_python_surface_cpu.py` in that checkout) and
committed unchanged; a change that means to move the surface regenerates it and says so."""
import inspect
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "python_surface.json")
MODULES = ("sdrgpu.filter", "sdrgpu.fft")


def surface():
    import importlib
    out = {}
    for modname in MODULES:
        mod = importlib.import_module(modname)
        for cname, cls in sorted(vars(mod).items()):
            if cname.startswith("_") or not inspect.isclass(cls) or cls.__module__ != modname:
                continue
            members = {}
            for name in sorted(n for n in dir(cls) if not n.startswith("_")):
                static = inspect.getattr_static(cls, name)
                if isinstance(static, property):
                    members[name] = "property"
                elif callable(getattr(cls, name)):
                    members[name] = str(inspect.signature(getattr(cls, name)))
                else:
                    members[name] = "attribute"
            out[f"{modname}.{cname}"] = {"init": str(inspect.signature(cls)), "members": members}
    return out


def test_python_surface_matches_golden(sdr):
    with open(GOLDEN) as f:
        golden = json.load(f)
    now = surface()
    assert sorted(now) == sorted(golden)
    for cname in golden:
        assert now[cname] == golden[cname], cname


if __name__ == "__main__":
    import conftest  # noqa: F401  (puts the package on sys.path)
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
