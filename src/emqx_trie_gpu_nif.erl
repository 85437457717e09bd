%%--------------------------------------------------------------------
%% emqx_trie_gpu_nif -- the NIF stubs of c_src/emqx_trie_gpu_nif.c (libemqx_gpumatch.so,
%% include/emqx_gpumatch.h).  Replaced at load time; every stub raises nif_not_loaded.
%%--------------------------------------------------------------------
-module(emqx_trie_gpu_nif).

-export([
    open/6,
    route_sync/2,
    route_set/3,
    route_set_many/3,
    route_dests/3,
    subscribers/3,
    register/3,
    alloc_handle/2,
    release_handle/3,
    reset_handles/1,
    set_local_node/2,
    sync_begin/1,
    sync_end/2,
    commit/1,
    snapshot_save/2,
    snapshot_load/2,
    empty/1,
    trie_member/2,
    route_member/2,
    match_async/3,
    publish_async/3,
    cancel/2,
    tune/3,
    stats/1,
    retain_open/2,
    retain_store/3,
    retain_delete/2,
    retain_clean/1,
    retain_commit/1,
    retain_match/3,
    retain_store/4,
    retain_tune/3,
    retain_match_limit/5,
    retain_clear_expired/2,
    retain_delete_matching/2,
    retain_page_read/5,
    match_rules/3,
    ruleset_open/2,
    ruleset_set/2,
    ruleset_match/2,
    ruleset_close/1,
    acl_open/2,
    acl_set/2,
    acl_match/2,
    acl_close/1,
    acldb_open/2,
    acldb_store/4,
    acldb_delete/3,
    acldb_purge/1,
    acldb_commit/1,
    acldb_match/2,
    acldb_close/1,
    share_open/2,
    share_subscribe/5,
    share_unsubscribe/4,
    share_down/2,
    share_strategy/3,
    share_commit/1,
    share_pick/2,
    share_members/3,
    share_close/1
]).

-on_load(init/0).

init() ->
    PrivDir =
        case code:priv_dir(emqx) of
            {error, _} -> "priv";
            Dir -> Dir
        end,
    erlang:load_nif(filename:join(PrivDir, "emqx_trie_gpu_nif"), 0).

-define(NOT_LOADED, erlang:nif_error(nif_not_loaded)).

%% open(Devices, WindowTopics, WindowBytes, WindowUs, MaxLevels,
%%      #{spin_us => N, bg_build => N, publish => boolean()}) -> {ok, Res} | {error, Reason}
open(_Devices, _WindowTopics, _WindowBytes, _WindowUs, _MaxLevels, _Opts) -> ?NOT_LOADED.
%% route_sync(Res, [{Filter, Present :: boolean()}]) -> {ok, Epoch}: set and committed (visible to
%% every later publish) before it returns; never waits for a background full build
route_sync(_Res, _Items) -> ?NOT_LOADED.
%% route_set(Res, Filter, Present :: boolean()) -> ok | {error, Reason} (pending until commit/1)
route_set(_Res, _Filter, _Present) -> ?NOT_LOADED.
%% route_set_many(Res, [Filter], Present) -> ok | {error, Reason} (a resync chunk, pending)
route_set_many(_Res, _Filters, _Present) -> ?NOT_LOADED.
%% route_dests(Res, [{Filter, [{NodeH, GroupH | none}]}], Commit :: boolean()) -> {ok, Epoch}
route_dests(_Res, _Items, _Commit) -> ?NOT_LOADED.
%% subscribers(Res, [{Filter, [SubH]}], Commit :: boolean()) -> {ok, Epoch}
subscribers(_Res, _Items, _Commit) -> ?NOT_LOADED.
%% register(Res, node | group | sub, [{Handle, Term}]) -> ok
register(_Res, _Kind, _Items) -> ?NOT_LOADED.

%% alloc_handle(Res, node | group | sub) -> {ok, N} | {error, e2big}
alloc_handle(_Res, _Kind) -> ?NOT_LOADED.

%% release_handle(Res, node | group | sub, N) -> ok | {error, enoent}
release_handle(_Res, _Kind, _N) -> ?NOT_LOADED.

%% reset_handles(Res) -> ok: every handle released (a restarted mirror's, whose table died)
reset_handles(_Res) -> ?NOT_LOADED.
%% set_local_node(Res, NodeH) -> ok
set_local_node(_Res, _NodeH) -> ?NOT_LOADED.
%% sync_begin(Res) -> {ok, Gen}
sync_begin(_Res) -> ?NOT_LOADED.
%% ---- the retainer's reverse match (emqx_retainer_mnesia.erl:138-195, 241-247) ----
%% retain_open(Device, IndexSpecs :: [[pos_integer()]]) -> {ok, R} | {error, Reason}
retain_open(_Device, _IndexSpecs) -> ?NOT_LOADED.
%% retain_store(R, Topic, ExpiryMs) -> ok (store_retained/2; 0: never expires)
retain_store(_R, _Topic, _ExpiryMs) -> ?NOT_LOADED.
%% retain_delete(R, Topic) -> ok (delete_message/2 of one topic)
retain_delete(_R, _Topic) -> ?NOT_LOADED.
%% retain_clean(R) -> ok (clean/1)
retain_clean(_R) -> ?NOT_LOADED.
%% retain_commit(R) -> ok: the mutations visible to retain_match/3
retain_commit(_R) -> ?NOT_LOADED.
%% retain_match(R, [Filter], NowMs) -> [[Topic]]: match_messages/3 for a batch of filters
retain_match(_R, _Filters, _NowMs) -> ?NOT_LOADED.
%% retain_store(R, Topic, ExpiryMs, TsMs) -> ok | {error, table_is_full}: store_retained/2 with
%% #message.timestamp and the table-full rule (emqx_retainer_mnesia.erl:141, :409-419)
retain_store(_R, _Topic, _ExpiryMs, _TsMs) -> ?NOT_LOADED.
%% retain_tune(R, delta_max | max_retained_messages, Value) -> ok
retain_tune(_R, _Key, _Value) -> ?NOT_LOADED.
%% retain_match_limit(R, [Filter], NowMs, [Limit], [Cursor]) -> {[[Topic]], [Cursor]}:
%% match_messages/3 with {Cursor, BatchNum} (:185-202); a cursor is a 16-byte binary, <<>> starts
retain_match_limit(_R, _Filters, _NowMs, _Limits, _Cursors) -> ?NOT_LOADED.
%% retain_clear_expired(R, NowMs) -> [Topic] (clear_expired/1, :154-164)
retain_clear_expired(_R, _NowMs) -> ?NOT_LOADED.
%% retain_delete_matching(R, Filter) -> [Topic] (delete_message/2 with wildcards, :166-180)
retain_delete_matching(_R, _Filter) -> ?NOT_LOADED.
%% retain_page_read(R, Filter | undefined, Page, Limit, NowMs) -> [Topic] (page_read/4, :204-238)
retain_page_read(_R, _Filter, _Page, _Limit, _NowMs) -> ?NOT_LOADED.
%% match_rules(Res, [Name], [{Filter, eq | words | binary}]) -> [Index | none]: the first rule
%% each name matches (emqx_authz_rule:match_topics/3, emqx_rewrite:match_and_rewrite/3)
match_rules(_Res, _Names, _Rules) -> ?NOT_LOADED.
%% ---- rule sets: every matching rule per name (emqx_rule_engine:get_rules_for_topic/1,
%% emqx_bridge:get_matched_egress_bridges/1, the exhook and trace topic filters) ----
%% ruleset_open(Device, WordHashBits :: 0) -> {ok, R} | {error, Reason}
ruleset_open(_Device, _WordHashBits) -> ?NOT_LOADED.
%% ruleset_set(R, [Rule :: [{Filter, eq | words | binary}]]) -> ok: replaces the whole list
ruleset_set(_R, _Rules) -> ?NOT_LOADED.
%% ruleset_match(R, [Name]) -> [[RuleIndex]]: per name the rules it matches, ascending, each once
ruleset_match(_R, _Names) -> ?NOT_LOADED.
%% ruleset_close(R) -> ok
ruleset_close(_R) -> ?NOT_LOADED.
%% ---- ACL lists: the first matching authz rule per request (emqx_authz_rule:matches/4 for
%% emqx_authz_file:authorize/4 and emqx_authz_mnesia:authorize/4) ----
%% acl_open(Device, WordHashBits :: 0) -> {ok, A} | {error, Reason}
acl_open(_Device, _WordHashBits) -> ?NOT_LOADED.
%% acl_set(A, [{allow | deny, Who, publish | subscribe | all, [{Filter, eq | words}]}]) -> ok:
%% replaces the whole list; Who = all | {username, Bin} | {clientid, Bin} | {slot, 0..63}
acl_set(_A, _Rules) -> ?NOT_LOADED.
%% acl_match(A, {[{ClientId | undefined, Username | undefined, WhoBits}],
%%               [{Name, ClientIndex, publish | subscribe}]}) -> [RuleIndex | none]
acl_match(_A, _ClientsAndRequests) -> ?NOT_LOADED.
%% acl_close(A) -> ok
acl_close(_A) -> ?NOT_LOADED.

%% The built-in authorization database (emqx_authz_mnesia) resident on the device.
%% acldb_open(Device, WordHashBits :: 0) -> {ok, D} | {error, Reason}
acldb_open(_Device, _WordHashBits) -> ?NOT_LOADED.
%% acldb_store(D, clientid | username | all, Key,
%%             [{allow | deny, publish | subscribe | all, Topic}]) -> ok:
%% store_rules/2; pending until acldb_commit/1
acldb_store(_D, _Kind, _Key, _Rules) -> ?NOT_LOADED.
%% acldb_delete(D, clientid | username | all, Key) -> ok: delete_rules/1
acldb_delete(_D, _Kind, _Key) -> ?NOT_LOADED.
%% acldb_purge(D) -> ok: purge_rules/0
acldb_purge(_D) -> ?NOT_LOADED.
%% acldb_commit(D) -> ok | {error, Reason}: makes the pending mutations visible
acldb_commit(_D) -> ?NOT_LOADED.
%% acldb_match(D, {[{ClientId | undefined, Username | undefined}],
%%                 [{Name, ClientIndex, publish | subscribe}]}) ->
%%     [{allow | deny, clientid | username | all, Position} | nomatch]: authorize/4 per request
acldb_match(_D, _ClientsAndRequests) -> ?NOT_LOADED.
%% acldb_close(D) -> ok
acldb_close(_D) -> ?NOT_LOADED.

%% Shared subscriptions (emqx_shared_sub): the membership resident on the device, pick/6 per
%% request.  Groups and subscribers are handles (alloc_handle/2).
%% share_open(Device, HashBits :: 0) -> {ok, S} | {error, Reason}
share_open(_Device, _HashBits) -> ?NOT_LOADED.
%% share_subscribe(S, Group, Topic, Sub, Local :: boolean()) -> ok: subscribe/3; pending until
%% share_commit/1.  Local = (erlang:node(SubPid) =:= node()).
share_subscribe(_S, _Group, _Topic, _Sub, _Local) -> ?NOT_LOADED.
%% share_unsubscribe(S, Group, Topic, Sub) -> ok: unsubscribe/3
share_unsubscribe(_S, _Group, _Topic, _Sub) -> ?NOT_LOADED.
%% share_down(S, Sub) -> ok: cleanup_down/1
share_down(_S, _Sub) -> ?NOT_LOADED.
%% share_strategy(S, Group | default, Strategy :: emqx_shared_sub:strategy()) -> ok
share_strategy(_S, _Group, _Strategy) -> ?NOT_LOADED.
%% share_commit(S) -> ok | {error, Reason}: makes the pending mutations visible
share_commit(_S) -> ?NOT_LOADED.
%% share_pick(S, [{Topic, Group, erlang:phash2(ClientId), erlang:phash2(SourceTopic),
%%                 Draw :: 0..16#FFFFFFFF, RoundRobinState | undefined}]) ->
%%     [{picked | no_subscribers | host_strategy, Sub | undefined, RoundRobinState | undefined,
%%       Count}]: pick/6 for a first dispatch per request; the state returned is stored back into
%%     {shared_sub_round_robin, Group, Topic}; host_strategy (sticky) is picked by the caller
%%     from share_members/3
share_pick(_S, _Requests) -> ?NOT_LOADED.
%% share_members(S, Group, Topic) -> [{Sub, Local :: boolean()}]: subscribers/2, in order
share_members(_S, _Group, _Topic) -> ?NOT_LOADED.
%% share_close(S) -> ok
share_close(_S) -> ?NOT_LOADED.
%% snapshot_save(Res, Path :: binary()) -> ok | {error, Reason}: the committed index to a file
snapshot_save(_Res, _Path) -> ?NOT_LOADED.
%% snapshot_load(Res, Path :: binary()) -> ok | {error, Reason}: into a fresh resource, no build
snapshot_load(_Res, _Path) -> ?NOT_LOADED.
%% sync_end(Res, Gen) -> {ok, Removed}
sync_end(_Res, _Gen) -> ?NOT_LOADED.
%% commit(Res) -> {ok, Epoch}
commit(_Res) -> ?NOT_LOADED.
empty(_Res) -> ?NOT_LOADED.
trie_member(_Res, _Filter) -> ?NOT_LOADED.
route_member(_Res, _Filter) -> ?NOT_LOADED.
%% match_async(Res, Topic, Ref) -> {ok, Call} | {error, e2big | ebusy | eshutdown}; later the
%% caller gets {emqx_trie_gpu, Ref, [Filter], ExactHit :: boolean()} | {emqx_trie_gpu, Ref, {error, R}}
match_async(_Res, _Topic, _Ref) -> ?NOT_LOADED.
%% publish_async(Res, Topic, Ref) -> {ok, Call} | {error, R}; later
%% {emqx_trie_gpu, Ref, {routes, [{To, Node | Group}], [{To, SubPid}]}} | {emqx_trie_gpu, Ref, {error, R}}
publish_async(_Res, _Topic, _Ref) -> ?NOT_LOADED.
%% cancel(Res, Call) -> true (never answered) | false (the answer is in the mailbox)
cancel(_Res, _Call) -> ?NOT_LOADED.
tune(_Res, _Key, _Value) -> ?NOT_LOADED.
stats(_Res) -> ?NOT_LOADED.
