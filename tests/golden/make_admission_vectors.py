"""Writes tests/golden/admission_vectors.json: the zone settings, calls and expected answers of the
reference's caps suite, transcribed as data.

  apps/emqx/test/emqx_mqtt_caps_SUITE.erl  t_check_pub (:27-43), t_check_sub (:45-72)
  apps/emqx/include/emqx_mqtt.hrl          the reason codes (:173-192)

A check_pub case is [flags, expected]; a check_sub case is [topic, subopts, expected]; expected is
"ok" or the reason code of {error, Code}.  `caps` holds what the test puts into the default zone;
every other key keeps the default of emqx_mqtt_caps.erl:61-72.  Run from the repository root:
python tests/golden/make_admission_vectors.py
"""
import json
import os

RC_TOPIC_FILTER_INVALID = 0x8F
RC_RETAIN_NOT_SUPPORTED = 0x9A
RC_QOS_NOT_SUPPORTED = 0x9B
RC_SHARED_SUBSCRIPTIONS_NOT_SUPPORTED = 0x9E
RC_WILDCARD_SUBSCRIPTIONS_NOT_SUPPORTED = 0xA2

SUBOPTS = {"rh": 0, "rap": 0, "nl": 0, "qos": 2}

VECTORS = {
    "source": "apps/emqx/test/emqx_mqtt_caps_SUITE.erl:27-72",
    "check_pub": {
        "caps": {"max_qos_allowed": 1, "retain_available": False},
        "cases": [
            [{"qos": 1, "retain": False}, "ok"],
            [{"qos": 2, "retain": False}, RC_QOS_NOT_SUPPORTED],
            [{"qos": 1, "retain": True}, RC_RETAIN_NOT_SUPPORTED],
        ],
    },
    "check_sub": {
        "caps": {"max_topic_levels": 2, "max_qos_allowed": 1, "shared_subscription": False,
                 "wildcard_subscription": False},
        "cases": [
            ["topic", SUBOPTS, "ok"],
            ["a/b/c/d", SUBOPTS, RC_TOPIC_FILTER_INVALID],
            ["+/#", SUBOPTS, RC_WILDCARD_SUBSCRIPTIONS_NOT_SUPPORTED],
            ["topic", dict(SUBOPTS, share=True), RC_SHARED_SUBSCRIPTIONS_NOT_SUPPORTED],
        ],
    },
}

if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "admission_vectors.json")
    with open(path, "w") as f:
        json.dump(VECTORS, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path)
