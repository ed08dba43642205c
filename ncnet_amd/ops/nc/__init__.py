"""The NeighConsensus execution paths behind ``ops/neigh_consensus.py``
(``select_path`` and the dispatcher live there; its docstring has the table).

Imports point downward only::

    layers   the single Conv4d layer, its wgrad launch geometry, shared helpers
    train    bf16 training stack (imports layers)
    x3       bf16x3 fp32-accurate paths (imports layers, train)
    fp8      e4m3 layer stack, fp8 weight cache and pins (imports layers)
    fused    fused (3,3)/(<=16,1) inference kernels (imports layers, fp8)

State that is rebound at run time is read only in the module that defines it:
``train.FAST1X``, ``x3._X3_DROP`` (ask ``x3_dropped``), ``fp8._FP8_PINS``
(hand tensors to ``fp8.pin``).
"""
