"""Writes tests/golden/authz_mnesia_vectors.json: the sample rule sets and expected answers of the
reference's built-in database suite, transcribed as data.

  apps/emqx_authz/test/emqx_authz_mnesia_SUITE.erl  t_username_topic_rules, t_clientid_topic_rules,
      t_all_topic_rules (:57-83: the three groups below, stored under each of the three key kinds by
      setup_client_samples/3, :141-161) and t_normalize_rules (:85-129)
  apps/emqx_authz/test/emqx_authz_test_lib.erl      test_no_topic_rules (:70-83),
      test_allow_topic_rules (:85-173), test_deny_topic_rules (:175-263)

A sample is [expected, action, topic]; expected is emqx_access_control:authorize/3's answer, which
is the group's no_match default when the source says nomatch.  Terms of t_normalize_rules are
written as tests/acl_ref.py term_from_json reads them ({"a": atom}, {"b": binary}, {"s": string},
{"t": tuple}, list).  Run from the repository root: python tests/golden/make_authz_mnesia_vectors.py
"""
import json
import os


def samples(kind):
    return [{"topics": ["eq test%s1/${username}" % k, "test%s2/${clientid}" % k, "test%s3/#" % k],
             "permission": kind, "action": a} for k, a in (("pub", "publish"), ("sub", "subscribe"), ("all", "all"))]


ALLOW = [
    # Publish rules
    ("deny", "publish", "testpub1/username"),
    ("allow", "publish", "testpub1/${username}"),
    ("allow", "publish", "testpub2/clientid"),
    ("allow", "publish", "testpub3/foobar"),
    ("deny", "publish", "testpub2/username"),
    ("deny", "publish", "testpub1/clientid"),
    ("deny", "subscribe", "testpub1/username"),
    ("deny", "subscribe", "testpub2/clientid"),
    ("deny", "subscribe", "testpub3/foobar"),
    # Subscribe rules
    ("deny", "subscribe", "testsub1/username"),
    ("allow", "subscribe", "testsub1/${username}"),
    ("allow", "subscribe", "testsub2/clientid"),
    ("allow", "subscribe", "testsub3/foobar"),
    ("allow", "subscribe", "testsub3/+/foobar"),
    ("allow", "subscribe", "testsub3/#"),
    ("deny", "subscribe", "testsub2/username"),
    ("deny", "subscribe", "testsub1/clientid"),
    ("deny", "subscribe", "testsub4/foobar"),
    ("deny", "publish", "testsub1/username"),
    ("deny", "publish", "testsub2/clientid"),
    ("deny", "publish", "testsub3/foobar"),
    # All rules
    ("deny", "subscribe", "testall1/username"),
    ("allow", "subscribe", "testall1/${username}"),
    ("allow", "subscribe", "testall2/clientid"),
    ("allow", "subscribe", "testall3/foobar"),
    ("allow", "subscribe", "testall3/+/foobar"),
    ("allow", "subscribe", "testall3/#"),
    ("deny", "publish", "testall1/username"),
    ("allow", "publish", "testall1/${username}"),
    ("allow", "publish", "testall2/clientid"),
    ("allow", "publish", "testall3/foobar"),
    ("deny", "subscribe", "testall2/username"),
    ("deny", "subscribe", "testall1/clientid"),
    ("deny", "subscribe", "testall4/foobar"),
    ("deny", "publish", "testall2/username"),
    ("deny", "publish", "testall1/clientid"),
    ("deny", "publish", "testall4/foobar"),
]
# test_deny_topic_rules lists the same requests in the same order with every answer the other one
FLIP = {"allow": "deny", "deny": "allow"}
DENY = [(FLIP[e], a, t) for e, a, t in ALLOW]


def tup(*xs):
    return {"t": list(xs)}


DOC = {
    "source": "emqx_authz_mnesia_SUITE.erl:57-129, emqx_authz_test_lib.erl:70-263",
    "client": {"clientid": "clientid", "username": "username", "peerhost": [127, 0, 0, 1]},
    "key_kinds": ["username", "clientid", "all"],
    "groups": [
        {"name": "no_topic_rules", "no_match": "deny", "rules": [],
         "samples": [["deny", "subscribe", "#"], ["deny", "subscribe", "subs"], ["deny", "publish", "pub"]]},
        {"name": "allow_topic_rules", "no_match": "deny", "rules": samples("allow"), "samples": [list(s) for s in ALLOW]},
        {"name": "deny_topic_rules", "no_match": "allow", "rules": samples("deny"), "samples": [list(s) for s in DENY]},
    ],
    "normalize_rules": {
        "who": tup({"a": "username"}, {"b": "username"}),
        "accepted": {"rules": [tup({"a": "allow"}, {"a": "publish"}, {"s": "t"})],
                     "sample": ["allow", "publish", "t"]},
        "refused": [
            {"rules": [[{"a": "allow"}, {"a": "publish"}, {"b": "t"}]], "error": "invalid_rule"},
            {"rules": [tup({"a": "allow"}, {"a": "pub"}, {"b": "t"})], "error": "invalid_rule_action"},
            {"rules": [tup({"a": "accept"}, {"a": "publish"}, {"b": "t"})], "error": "invalid_rule_permission"},
        ],
    },
}

if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "authz_mnesia_vectors.json")
    with open(out, "w") as f:
        json.dump(DOC, f, indent=1)
        f.write("\n")
    print(out)
