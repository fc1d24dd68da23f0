"""The experiments of the reference's own demos and tests, as model functions: which of them models.from_function
can put on the device.  tests/_demo_models.py holds this project's model of each (the reference's code is not in this
repository); each is first held to what the reference's own function returns on the same seeded inputs
(golden/demo_model_functions.npz, made by golden/make_golden.py from the reference's source tree), to rounding, and
the translation is then checked against the function itself, bit for bit."""
import os

import numpy as np

import _demo_models

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "demo_model_functions.npz")


def test_reference_demo_model_functions_translate():
    from optbayesexpt_amd import _exprmodel, _fnmodel
    golden = np.load(GOLDEN)
    table = _demo_models.demo_models()
    keys = [str(k) for k in golden["keys"]]
    assert sorted(keys) == sorted(table)                  # a model here for every model function of the reference
    verdicts = {}
    for k, key in enumerate(keys):
        fn = table[key][0]
        # the model computes what the reference's own function computed, to rounding
        ref = golden[f"out_{k}"]
        np.testing.assert_allclose(np.asarray(fn(*_demo_models.demo_inputs(key)), dtype=np.float64), ref,
                                   rtol=1e-12, atol=1e-13 * np.abs(ref).max(), err_msg=key)
        try:
            exprs, s, p, c = _fnmodel.expressions_from_function(fn)
            _, numpy_form, _ = _exprmodel.translate(exprs, s, p, c)
            _fnmodel.check_against_function(fn, numpy_form, len(s), len(p), len(c))
            verdicts[key] = "device"
        except ValueError as exc:
            verdicts[key] = f"host ({exc})"
    on_device = {k for k, v in verdicts.items() if v == "device"}
    print("\n".join(f"{k}: {v}" for k, v in sorted(verdicts.items())))
    # the model of every real-arithmetic demo is translatable ...
    for demo in ("demos/find_peak/sequentialLorentzian.py", "demos/sweeper/sweeper.py", "demos/pipulse/pipulse.py",
                 "demos/line_plus_noise/line_plus_noise.py", "demos/fit_vs_obe/fit_vs_obe_makedata.py",
                 "demos/find_peak/seqLor_pdfevolve.py", "demos/server/server_script.py"):
        assert any(k.startswith(demo) for k in on_device), (demo, verdicts)
    # ... the complex-impedance coil model is not, and says why
    coil = [v for k, v in verdicts.items() if k.startswith("demos/lockin/lockin_of_coil.py")]
    assert coil and all(v.startswith("host") for v in coil)
