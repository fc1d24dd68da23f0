"""The expression model of the batch-update tests' conjugate case (pre-built by __graft_entry__.build(), like the
models of _expr_models.py, so that its plugin library travels with the repository snapshot)."""


def expression_models():
    from optbayesexpt_amd import models
    # linear in its parameters: with a Gaussian prior and Gaussian noise the posterior has a closed form
    return {"line": models.from_expression("a + b*x", settings=("x",), parameters=("a", "b"))}
