"""The reference semantics of the admission pass (emqxgm_admit_*, DESIGN.md 6b "Admission"),
restated for the tests from the reference's text, clause by clause.  Test-only: nothing here is
shared with emqx_amd/csrc/gm_admit_match.h, which scans bytes eight at a time; this walks word
lists and lets Python's strict ``utf-8`` decoder say what ``<<C/utf8, _/binary>>`` accepts.

* ``validate``  emqx_topic:validate/2, apps/emqx/src/emqx_topic.erl:98-130
* ``parse``     emqx_topic:parse/2, :212-233
* ``levels`` / ``wildcard``  :151-153, :54-64
* ``check_pub`` / ``check_sub``  emqx_mqtt_caps:do_check_pub / do_check_sub,
  apps/emqx/src/emqx_mqtt_caps.erl:94-105, 134-152; defaults :61-72; reason codes
  apps/emqx/include/emqx_mqtt.hrl:173-192
* ``reason``    the order of the channel: emqx_packet:check/1 (emqx_packet.erl:254-273), parse
  inside handle_in (emqx_channel.erl:510), check_pub_caps / check_sub_caps (:647, :801)

The ``/utf8`` rule is OTP's (the Erlang reference manual's bit syntax: RFC 3629 -- no overlong
forms, no surrogates, nothing above U+10FFFF; U+FFFE and U+FFFF are legal); no Erlang ran to make
these tests, Python's decoder rejects the same set.  A sequence ``/utf8`` does not accept ends
validate3 in ``function_clause`` (no clause of :125-130 matches)."""
MAX_TOPIC_LEN = 65535
NONE = 0xFFFFFFFF

V_NAMES = ("ok", "empty_topic", "topic_too_long", "topic_name_error", "topic_invalid_#", "topic_invalid_char",
           "function_clause")
V = {n: i for i, n in enumerate(V_NAMES)}
P_OK, P_INVALID = 0, 1
F_WILDCARD, F_SHARED, F_EXCLUSIVE, F_EXCL_LOOKUP = 1 << 24, 1 << 25, 1 << 26, 1 << 27
NAME, FILTER = 0, 1
IN_RETAIN, IN_HAS_SHARE = 4, 8
RC_TOPIC_FILTER_INVALID, RC_TOPIC_NAME_INVALID = 0x8F, 0x90
RC_RETAIN_NOT_SUPPORTED, RC_QOS_NOT_SUPPORTED = 0x9A, 0x9B
RC_SHARED_SUBSCRIPTIONS_NOT_SUPPORTED, RC_WILDCARD_SUBSCRIPTIONS_NOT_SUPPORTED = 0x9E, 0xA2
RAISES = 0x100

DEFAULT_CAPS = dict(max_topic_levels=65535, max_qos_allowed=2, retain_available=True, wildcard_subscription=True,
                    shared_subscription=True, exclusive_subscription=False)  # emqx_mqtt_caps.erl:61-72


def caps(**kw):
    c = dict(DEFAULT_CAPS)
    c.update(kw)
    return c


class TopicError(Exception):
    pass


def words(topic: bytes):
    """:162-169: binaries; the atoms '', '+' and '#' as the strings "''", "'+'", "'#'"."""
    return [{b"": "''", b"+": "'+'", b"#": "'#'"}.get(w, w) for w in topic.split(b"/")]


def levels(topic: bytes) -> int:
    return len(topic.split(b"/"))


def wildcard(ws) -> bool:
    return any(w in ("'+'", "'#'") for w in ws)


def _validate3(w: bytes):
    """:125-130, code point by code point from the left."""
    p = 0
    while p < len(w):
        n = 1  # the prefix of 1..4 bytes that is one code point
        while True:
            try:
                c = w[p:p + n].decode("utf-8", "strict")
                break
            except UnicodeDecodeError:
                n += 1
                if n > 4 or p + n > len(w):
                    raise TopicError("function_clause")
        if c in "#+\0":
            raise TopicError("topic_invalid_char")
        p += n
    return True


def _validate2(ws):
    """:111-123."""
    for i, w in enumerate(ws):
        if w == "'#'":
            if i == len(ws) - 1:
                return True
            raise TopicError("topic_invalid_#")
        if w in ("''", "'+'"):
            continue
        _validate3(w)
    return True


def validate(kind: str, topic: bytes):
    """True, or the error's name."""
    try:
        if topic == b"":
            raise TopicError("empty_topic")
        if len(topic) > MAX_TOPIC_LEN:
            raise TopicError("topic_too_long")
        ws = words(topic)
        if kind == "filter":
            return _validate2(ws)
        assert kind == "name"
        if _validate2(ws) and not wildcard(ws):
            return True
        raise TopicError("topic_name_error")
    except TopicError as e:
        return e.args[0]


def parse(topic_filter: bytes, options=None):
    """(Topic, Options), or None for error({invalid_topic_filter, _})."""
    options = dict(options or {})
    if topic_filter.startswith(b"$share/"):
        if "share" in options:  # :213-214
            return None
        rest = topic_filter[7:]
        parts = rest.split(b"/", 1)
        if len(parts) == 1:  # [_Any]
            return None
        share_name, filt = parts
        if b"+" in share_name or b"#" in share_name:
            return None
        options["share"] = share_name
        return parse(filt, options)
    if topic_filter.startswith(b"$exclusive/"):  # :225-231
        topic = topic_filter[11:]
        if topic == b"":
            return None
        options["is_exclusive"] = True
        return topic, options
    return topic_filter, options


def check_pub(topic: bytes, qos: int, retain: bool, c) -> int:
    """do_check_pub with topic_levels = levels(Topic)."""
    if c["max_topic_levels"] > 0 and levels(topic) > c["max_topic_levels"]:
        return RC_TOPIC_NAME_INVALID
    if qos > c["max_qos_allowed"]:
        return RC_QOS_NOT_SUPPORTED
    if retain and not c["retain_available"]:
        return RC_RETAIN_NOT_SUPPORTED
    return 0


def check_sub(topic: bytes, subopts, c):
    """(reason code, whether the clause that asks emqx_exclusive_subscription was reached)."""
    if c["max_topic_levels"] > 0 and levels(topic) > c["max_topic_levels"]:
        return RC_TOPIC_FILTER_INVALID, False
    if wildcard(words(topic)) and not c["wildcard_subscription"]:
        return RC_WILDCARD_SUBSCRIPTIONS_NOT_SUPPORTED, False
    if "share" in subopts and not c["shared_subscription"]:
        return RC_SHARED_SUBSCRIPTIONS_NOT_SUPPORTED, False
    if subopts.get("is_exclusive", False) and not c["exclusive_subscription"]:
        return RC_TOPIC_FILTER_INVALID, False
    if subopts.get("is_exclusive", False):
        return 0, True
    return 0, False


def record(mode: int, item: bytes, in_flags: int = 0, c=None):
    """The four words emqxgm_admit_batch answers for the item (include/emqx_gpumatch.h)."""
    c = DEFAULT_CAPS if c is None else c
    v = validate("name" if mode == NAME else "filter", item)
    w0 = 0 if v is True else V[v]
    if mode == NAME:
        if len(item) > MAX_TOPIC_LEN:
            return (w0, 0, 0, NONE)
        rc = check_pub(item, in_flags & 3, bool(in_flags & IN_RETAIN), c)
        flags = F_WILDCARD if wildcard(words(item)) else 0
        return (w0 | rc << 16 | flags, levels(item), 0, NONE)
    opts = {"share": True} if in_flags & IN_HAS_SHARE else {}
    p = parse(item, opts)
    if p is None:
        return (w0 | P_INVALID << 8, 0, 0, NONE)
    topic, o = p
    assert item.endswith(topic)
    share = o.get("share")
    if len(item) > MAX_TOPIC_LEN:  # parse's answer alone: levels, wildcard and caps are not run
        return (w0 | (F_SHARED if "share" in o else 0) | (F_EXCLUSIVE if o.get("is_exclusive") else 0), 0,
                len(item) - len(topic), len(share) if isinstance(share, bytes) else NONE)
    rc, lookup = check_sub(topic, o, c)
    flags = (F_WILDCARD if wildcard(words(topic)) else 0) | (F_SHARED if "share" in o else 0) | \
        (F_EXCLUSIVE if o.get("is_exclusive") else 0) | (F_EXCL_LOOKUP if lookup else 0)
    return (w0 | rc << 16 | flags, levels(topic), len(item) - len(topic),
            len(share) if isinstance(share, bytes) else NONE)


def reason(mode: int, rec) -> int:
    """The first failure in the channel's order."""
    if rec[0] & 0xFF:
        return RC_TOPIC_NAME_INVALID if mode == NAME else RC_TOPIC_FILTER_INVALID
    if (rec[0] >> 8) & 0xFF:
        return RAISES
    return (rec[0] >> 16) & 0xFF


def subscribe_packet_check(filters):
    """emqx_packet:check/1 of a SUBSCRIBE (emqx_packet.erl:267-273, 411-420): 0, or 16#8F for an
    empty list or any filter validate/1 refuses."""
    if not filters:
        return RC_TOPIC_FILTER_INVALID
    return 0 if all(validate("filter", f) is True for f in filters) else RC_TOPIC_FILTER_INVALID
