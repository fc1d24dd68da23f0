"""The expression model of the own-noise batch tests' crafted values (pre-built by __graft_entry__.build(), like the
models of _expr_models.py, so that its plugin library travels with the repository snapshot)."""


def expression_models():
    from optbayesexpt_amd import models
    # the output is a parameter row: a test sets every model value it wants, 0, 1, NaN and 700 included
    return {"row": models.from_expression("q", settings=("x",), parameters=("q",))}
