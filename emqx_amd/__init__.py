"""emqx_amd -- MI355X-native batched MQTT topic matching behind the EMQX routing API.

The product is ``libemqx_gpumatch.so`` (gfx950 HIP kernels + host index builder + C-ABI,
``include/emqx_gpumatch.h``).  This package is the host-side mirror of the reference's
``emqx_trie`` / ``emqx_router`` / ``emqx_broker`` (publish fan-out) modules over that library:

    from emqx_amd import Trie, Router, Broker, Engine
"""
from . import authz  # noqa: F401
from .admission import Admission  # noqa: F401
from .authz import AclList, BuiltinDb, InvalidRule  # noqa: F401
from .broker import Broker  # noqa: F401
from .engine import NONE, Acl, AclDb, SharedSub, AsyncMatcher, AsyncResult, Batcher, DeviceResult, Engine, EngineError, MatchResult, PublishResult, Window  # noqa: F401
from .router import Router, SessionRouter  # noqa: F401
from .retainer import Retainer  # noqa: F401
from .rules import TopicRules  # noqa: F401
from .shared_sub import SharedSubs  # noqa: F401
from .ruleset import RuleSet, get_matched_egress_bridges, get_rules_for_topic  # noqa: F401
from .trie import Trie  # noqa: F401

__all__ = ["Engine", "EngineError", "MatchResult", "DeviceResult", "PublishResult", "Trie",
           "Router", "SessionRouter", "Broker", "TopicRules", "RuleSet", "Acl", "AclList", "authz",
           "AclDb", "BuiltinDb", "InvalidRule", "SharedSub", "SharedSubs", "Admission",
           "get_rules_for_topic", "get_matched_egress_bridges", "Retainer", "Batcher", "Window",
           "AsyncMatcher", "AsyncResult", "NONE"]
