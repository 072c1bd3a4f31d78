"""No code: the names ``lib`` and ``Device`` of the former Twin-L2O binding, kept importable for a caller written before the
library was folded into ``libl2o_hip.so``.  There is one library and one loader -- the entry points of
``include/l2o_twin_abi.h`` are in ``_abi.PROTOTYPES``, errors go through ``_abi.check`` -- and the marshalling is
``_engine.TwinDevice``.  Nothing in this tree imports this module; new code imports those."""
from ._abi import lib  # noqa: F401
from ._engine import TwinDevice as Device  # noqa: F401
