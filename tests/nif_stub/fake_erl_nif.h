/* Test infrastructure only: what the fake erl_nif runtime (fake_erl_nif.c) offers the driver
 * beyond erl_nif's own calls.
 *
 * Terms.  Atoms, pids, [] and the badarg exception are immediates: an atom name gives the same
 * ERL_NIF_TERM in every environment, process-wide.  Every other term is one malloc'ed cell owned
 * by the environment that made it; enif_clear_env / enif_free_env free the cells, so a term used
 * after its environment is a heap-use-after-free under AddressSanitizer.  A resource term holds
 * one reference of its resource and drops it when its environment goes.
 *
 * Balance.  The runtime counts live environments and live resources per type; a release of a
 * resource that is not live aborts with a message. */
#ifndef FAKE_ERL_NIF_H
#define FAKE_ERL_NIF_H
#include <stdio.h>

#include "erl_nif.h"

#define FAKE_MAX_PIDS 4096
#define FAKE_BADARG ((ERL_NIF_TERM)0x7)
#define FAKE_NIL ((ERL_NIF_TERM)0x5)

/* the environment of one NIF call made by process `pid` (enif_self); freed by enif_free_env when
 * the call has returned */
ErlNifEnv* fake_call_env(unsigned pid);
ERL_NIF_TERM fake_make_pid(unsigned pid);
ERL_NIF_TERM fake_make_ref(ErlNifEnv* env); /* make_ref/0: unique */
ERL_NIF_TERM fake_make_ref_id(ErlNifEnv* env, unsigned long id);
ERL_NIF_TERM fake_make_binary(ErlNifEnv* env, const void* p, size_t n);
ERL_NIF_TERM fake_make_tuple_arr(ErlNifEnv* env, unsigned n, const ERL_NIF_TERM* a);
ERL_NIF_TERM fake_make_map(ErlNifEnv* env, unsigned n, const ERL_NIF_TERM* k, const ERL_NIF_TERM* v);
int fake_term_eq(ERL_NIF_TERM a, ERL_NIF_TERM b);
void fake_print(FILE* f, ERL_NIF_TERM t);
/* One message of `pid`'s mailbox, waiting up to timeout_ms: 1 and the message in an environment
 * the caller frees, or 0. */
int fake_recv(unsigned pid, int timeout_ms, ErlNifEnv** env, ERL_NIF_TERM* msg);
long fake_live_envs(void);
/* live resources of type i (0 .. fake_resource_types() - 1) and its name */
int fake_resource_types(void);
long fake_live_resources(int i, const char** name);
#endif
