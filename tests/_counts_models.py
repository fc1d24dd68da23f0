"""The two-channel expression models of the count-scoring tests (pre-built by __graft_entry__.build(), like the models
of _expr_models.py, so that their plugin libraries travel with the repository snapshot)."""
import _binomial_oracle
import _poisson_oracle


def expression_models():
    from optbayesexpt_amd import models
    return {"decays": models.from_expression(_poisson_oracle.DECAYS, settings=("t",), parameters=("a", "b", "T1")),
            "ramsey": models.from_expression(_binomial_oracle.RAMSEY, settings=("t",), parameters=("f", "T2"))}
