/* nif_driver.c -- TEST INFRASTRUCTURE: runs c_src/emqx_trie_gpu_nif.c on the fake erl_nif runtime
 * (tests/nif_stub/fake_erl_nif.c).  It calls nif_init() and load, then executes the script on
 * stdin, one line each (terms in the text format of tests/nif_terms.py; $name is a bound name):
 *
 *   call PID NAME/ARITY BIND [Arg, ...]   a table entry called as fake process PID; prints
 *                                         "= Result".  BIND is - or a name that gets X of a result
 *                                         {ok, X}, else the whole result (and BIND_1 .. BIND_n the
 *                                         elements, when that is a tuple).  The call's environment
 *                                         is freed when it has returned.
 *   recv PID MS BIND                      one message of PID's mailbox within MS milliseconds:
 *                                         "< Message" or "< timeout"
 *   ref NAME                              a fresh reference (make_ref/0), printed as "= &N"
 *   drop NAME                             forgets a name (a resource loses that reference)
 *   rc N / rc_create N                    what the mocks and null stubs below the NIF return
 *                                         (CPU builds; 0 = work)
 *   sleep MS
 *   balance                               "B ..." lines as at exit, names and mailboxes aside
 *   load RES THREADS CALLS CANCEL_PCT SEED [Topic, ...]
 *                                         the concurrent load: THREADS publisher processes (pids
 *                                         1000 ..) call match_async one topic at a time, wait for
 *                                         the message, cancel CANCEL_PCT % of the calls after a
 *                                         random while and cancel every call a second time, while
 *                                         process 999 runs alloc_handle / register / release_handle.
 *                                         Prints "M TopicIndex Message" per message and "LOAD
 *                                         accepted A answered N cancelled C refused R violations V
 *                                         live_calls L"; a violation (also printed, "V ...") is a
 *                                         call answered twice, not at all, after a cancel that
 *                                         returned true, or a second cancel that returned true.
 *
 * At exit every name is dropped, the mailboxes are drained, and the driver prints the function
 * table ("T name/arity calls"), "B mailbox N" (messages nobody received), "B res TYPE N" (live
 * resources per type) and "B envs N" (live environments).  The documented balance is all zero
 * once every name is dropped -- the term environments of a resource's handle tables go with the
 * resource -- and anything else makes the exit status 3. */
#define _GNU_SOURCE
#include <ctype.h>
#include <errno.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "fake_erl_nif.h"

ErlNifEntry* nif_init(void);
extern int g_stub_rc __attribute__((weak));
extern int g_stub_create_rc __attribute__((weak));

#define FAIL(...)                               \
  do {                                          \
    fflush(stdout);                             \
    fprintf(stderr, "nif_driver: " __VA_ARGS__); \
    fprintf(stderr, "\n");                      \
    exit(2);                                    \
  } while (0)

static ErlNifEntry* g_entry;
static unsigned long* g_calls; /* per table entry */

typedef struct {
  char name[32];
  ErlNifEnv* env;
  ERL_NIF_TERM t;
} var;
static var g_vars[4096];
static int g_nvars;

static var* find_var(const char* name, size_t n) {
  for (int i = 0; i < g_nvars; ++i)
    if (strlen(g_vars[i].name) == n && !memcmp(g_vars[i].name, name, n)) return &g_vars[i];
  return NULL;
}

static void drop_var(const char* name) {
  var* v = find_var(name, strlen(name));
  if (!v) return;
  enif_free_env(v->env);
  *v = g_vars[--g_nvars];
}

static void bind_var(const char* name, ERL_NIF_TERM t) {
  drop_var(name);
  if (g_nvars == 4096 || strlen(name) >= sizeof g_vars[0].name) FAIL("too many names, or too long: %s", name);
  var* v = &g_vars[g_nvars++];
  strcpy(v->name, name);
  v->env = enif_alloc_env();
  v->t = enif_make_copy(v->env, t);
}

/* ---- the parser ---- */
static void skip_ws(const char** p) {
  while (**p == ' ' || **p == '\t') ++*p;
}

static int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

static ERL_NIF_TERM parse(ErlNifEnv* env, const char** p);

/* elements up to `close`; returns the count (terms malloc'ed in *out) */
static unsigned parse_seq(ErlNifEnv* env, const char** p, char close, char alt, ERL_NIF_TERM** out) {
  unsigned n = 0, cap = 8;
  ERL_NIF_TERM* v = malloc(sizeof *v * cap);
  skip_ws(p);
  while (**p != close && **p != alt) {
    if (n == cap) v = realloc(v, sizeof *v * (cap *= 2));
    v[n++] = parse(env, p);
    skip_ws(p);
    if (**p == ',') {
      ++*p;
      skip_ws(p);
    } else if (**p != close && **p != alt) {
      FAIL("expected , or %c at: %.20s", close, *p);
    }
  }
  *out = v;
  return n;
}

static ERL_NIF_TERM parse(ErlNifEnv* env, const char** p) {
  skip_ws(p);
  const char* s = *p;
  if (*s == '{') {
    ERL_NIF_TERM* v;
    ++*p;
    const unsigned n = parse_seq(env, p, '}', '}', &v);
    ++*p;
    const ERL_NIF_TERM t = fake_make_tuple_arr(env, n, v);
    free(v);
    return t;
  }
  if (*s == '[') {
    ERL_NIF_TERM* v;
    ++*p;
    const unsigned n = parse_seq(env, p, ']', '|', &v);
    ERL_NIF_TERM tail = FAKE_NIL;
    if (**p == '|') {
      ++*p;
      tail = parse(env, p);
      skip_ws(p);
      if (**p != ']') FAIL("expected ] at: %.20s", *p);
    }
    ++*p;
    for (unsigned i = n; i-- > 0;) tail = enif_make_list_cell(env, v[i], tail);
    free(v);
    return tail;
  }
  if (s[0] == '#' && s[1] == '{') {
    unsigned n = 0, cap = 8;
    ERL_NIF_TERM *k = malloc(sizeof *k * cap), *v = malloc(sizeof *v * cap);
    *p += 2;
    skip_ws(p);
    while (**p != '}') {
      if (n == cap) {
        cap *= 2;
        k = realloc(k, sizeof *k * cap);
        v = realloc(v, sizeof *v * cap);
      }
      k[n] = parse(env, p);
      skip_ws(p);
      if ((*p)[0] != '=' || (*p)[1] != '>') FAIL("expected => at: %.20s", *p);
      *p += 2;
      v[n++] = parse(env, p);
      skip_ws(p);
      if (**p == ',') ++*p;
      skip_ws(p);
    }
    ++*p;
    const ERL_NIF_TERM t = fake_make_map(env, n, k, v);
    free(k);
    free(v);
    return t;
  }
  if (s[0] == '<' && s[1] == '<') {
    const char* q = s + 2;
    size_t n = 0;
    while (hexval(q[2 * n]) >= 0 && hexval(q[2 * n + 1]) >= 0) ++n;
    if (q[2 * n] != '>' || q[2 * n + 1] != '>') FAIL("bad binary at: %.20s", s);
    ERL_NIF_TERM t;
    unsigned char* d = enif_make_new_binary(env, n, &t);
    for (size_t i = 0; i < n; ++i) d[i] = (unsigned char)(hexval(q[2 * i]) * 16 + hexval(q[2 * i + 1]));
    *p = q + 2 * n + 2;
    return t;
  }
  if (*s == '&' || *s == '@') {
    char* end;
    const unsigned long id = strtoul(s + 1, &end, 10);
    if (end == s + 1) FAIL("bad reference or pid at: %.20s", s);
    *p = end;
    return *s == '&' ? fake_make_ref_id(env, id) : fake_make_pid((unsigned)id);
  }
  if (*s == '$') {
    const char* q = s + 1;
    while (isalnum((unsigned char)*q) || *q == '_') ++q;
    var* v = find_var(s + 1, (size_t)(q - s - 1));
    if (!v) FAIL("unbound name at: %.20s", s);
    *p = q;
    return enif_make_copy(env, v->t);
  }
  if (*s == '\'') {
    const char* q = strchr(s + 1, '\'');
    if (!q) FAIL("unterminated atom");
    char* name = strndup(s + 1, (size_t)(q - s - 1));
    const ERL_NIF_TERM t = enif_make_atom(env, name);
    free(name);
    *p = q + 1;
    return t;
  }
  if (*s == '-' || isdigit((unsigned char)*s)) {
    char* end;
    const char* q = s + (*s == '-');
    while (isdigit((unsigned char)*q)) ++q;
    if (*q == '.' || *q == 'e') {
      const double d = strtod(s, &end);
      *p = end;
      return enif_make_double(env, d);
    }
    errno = 0;
    if (*s == '-') {
      const long l = strtol(s, &end, 10);
      if (errno) FAIL("integer out of range at: %.24s", s);
      *p = end;
      return enif_make_int64(env, l);
    }
    const unsigned long u = strtoul(s, &end, 10);
    if (errno) FAIL("integer out of range at: %.24s", s);
    *p = end;
    return enif_make_uint64(env, u);
  }
  if (*s >= 'a' && *s <= 'z') {
    const char* q = s;
    while (isalnum((unsigned char)*q) || *q == '_' || *q == '@') ++q;
    char* name = strndup(s, (size_t)(q - s));
    const ERL_NIF_TERM t = enif_make_atom(env, name);
    free(name);
    *p = q;
    return t;
  }
  FAIL("cannot parse a term at: %.20s", s);
  return 0;
}

/* ---- calls ---- */
static int find_fn(const char* name, unsigned arity) {
  for (int i = 0; i < g_entry->num_of_funcs; ++i)
    if (!strcmp(g_entry->funcs[i].name, name) && g_entry->funcs[i].arity == arity) return i;
  return -1;
}

static ERL_NIF_TERM call_fn(int fn, ErlNifEnv* env, unsigned argc, const ERL_NIF_TERM* argv) {
  __atomic_fetch_add(&g_calls[fn], 1, __ATOMIC_RELAXED);
  return g_entry->funcs[fn].fptr(env, (int)argc, argv);
}

/* X of {ok, X}, else t itself */
static ERL_NIF_TERM ok_value(ErlNifEnv* env, ERL_NIF_TERM t) {
  int ar;
  const ERL_NIF_TERM* el;
  if (enif_get_tuple(env, t, &ar, &el) && ar == 2 && el[0] == enif_make_atom(env, "ok")) return el[1];
  return t;
}

static char* next_word(char** p) {
  while (**p == ' ') ++*p;
  char* w = *p;
  while (**p && **p != ' ') ++*p;
  if (**p) *(*p)++ = 0;
  return w;
}

static void do_call(char* rest) {
  const unsigned pid = (unsigned)atoi(next_word(&rest));
  char* fn = next_word(&rest);
  char* bind = next_word(&rest);
  char* slash = strchr(fn, '/');
  if (!slash) FAIL("call: NAME/ARITY expected, got %s", fn);
  *slash = 0;
  const unsigned arity = (unsigned)atoi(slash + 1);
  const int f = find_fn(fn, arity);
  if (f < 0) FAIL("no table entry %s/%u", fn, arity);
  ErlNifEnv* env = fake_call_env(pid);
  const char* p = rest;
  ERL_NIF_TERM argv[16], l = parse(env, &p), h;
  unsigned argc = 0;
  while (enif_get_list_cell(env, l, &h, &l)) {
    if (argc == 16) FAIL("too many arguments");
    argv[argc++] = h;
  }
  if (argc != arity) FAIL("%s/%u called with %u arguments", fn, arity, argc);
  const ERL_NIF_TERM r = call_fn(f, env, argc, argv);
  fputs("= ", stdout);
  fake_print(stdout, r);
  fputc('\n', stdout);
  if (strcmp(bind, "-")) {
    const ERL_NIF_TERM v = ok_value(env, r);
    int ar;
    const ERL_NIF_TERM* el;
    bind_var(bind, v);
    if (enif_get_tuple(env, v, &ar, &el)) /* NAME_1 .. NAME_n: the elements of a tuple */
      for (int i = 0; i < ar && i < 9; ++i) {
        char name[40];
        snprintf(name, sizeof name, "%.28s_%d", bind, i + 1);
        bind_var(name, el[i]);
      }
  }
  enif_free_env(env);
}

static void do_recv(char* rest) {
  const unsigned pid = (unsigned)atoi(next_word(&rest));
  const int ms = atoi(next_word(&rest));
  char* bind = next_word(&rest);
  ErlNifEnv* env;
  ERL_NIF_TERM t;
  if (!fake_recv(pid, ms, &env, &t)) {
    puts("< timeout");
    return;
  }
  fputs("< ", stdout);
  fake_print(stdout, t);
  fputc('\n', stdout);
  if (*bind && strcmp(bind, "-")) bind_var(bind, t);
  enif_free_env(env);
}

static long drain_mailboxes(void) {
  long n = 0;
  ErlNifEnv* env;
  ERL_NIF_TERM t;
  for (unsigned pid = 1; pid < FAKE_MAX_PIDS; ++pid)
    while (fake_recv(pid, 0, &env, &t)) {
      ++n;
      enif_free_env(env);
    }
  return n;
}

static int print_balance(long ignore_envs) {
  int bad = 0;
  for (int i = 0; i < fake_resource_types(); ++i) {
    const char* name;
    const long n = fake_live_resources(i, &name);
    printf("B res %s %ld\n", name, n);
    bad |= n != 0;
  }
  const long e = fake_live_envs() - ignore_envs;
  printf("B envs %ld\n", e);
  return bad | (e != 0);
}

/* ---- the concurrent load ---- */
typedef struct {
  unsigned k, calls, cancel_pct, seed, ntopics;
  ERL_NIF_TERM res; /* in an environment that outlives the threads */
  const ERL_NIF_TERM* topics;
  unsigned long accepted, answered, cancelled, refused, violations;
} load_thread;

static pthread_mutex_t g_out_mu = PTHREAD_MUTEX_INITIALIZER;
static int g_stop_writer;
static int F_MATCH, F_CANCEL, F_ALLOC, F_REGISTER, F_RELEASE;

static unsigned rnd(unsigned* s) {
  *s = *s * 1664525u + 1013904223u;
  return *s >> 8;
}

static void violation(load_thread* t, unsigned i, const char* what) {
  pthread_mutex_lock(&g_out_mu);
  printf("V thread %u call %u: %s\n", t->k, i, what);
  pthread_mutex_unlock(&g_out_mu);
  t->violations++;
}

/* the message of call `ref` from pid's mailbox (it must be the next one), printed */
static int take_message(load_thread* t, unsigned i, unsigned pid, unsigned ti, ERL_NIF_TERM ref) {
  ErlNifEnv* me;
  ERL_NIF_TERM m;
  int ar;
  const ERL_NIF_TERM* el;
  if (!fake_recv(pid, 20000, &me, &m)) {
    violation(t, i, "no message within the limit");
    return 0;
  }
  if (!enif_get_tuple(me, m, &ar, &el) || ar < 3 || !fake_term_eq(el[1], ref))
    violation(t, i, "a message that is not this call's (answered twice, or after a cancel)");
  pthread_mutex_lock(&g_out_mu);
  printf("M %u ", ti);
  fake_print(stdout, m);
  fputc('\n', stdout);
  pthread_mutex_unlock(&g_out_mu);
  enif_free_env(me);
  t->answered++;
  return 1;
}

static void* load_run(void* arg) {
  load_thread* t = arg;
  const unsigned pid = 1000 + t->k;
  unsigned s = t->seed * 7919u + t->k;
  const ERL_NIF_TERM a_true = enif_make_atom(NULL, "true"), a_false = enif_make_atom(NULL, "false");
  for (unsigned i = 0; i < t->calls; ++i) {
    const unsigned ti = rnd(&s) % t->ntopics;
    ErlNifEnv* keep = enif_alloc_env(); /* this process's own heap: the reference and the call */
    const ERL_NIF_TERM ref = fake_make_ref(keep);
    ErlNifEnv* env = fake_call_env(pid);
    ERL_NIF_TERM argv[3] = {enif_make_copy(env, t->res), enif_make_copy(env, t->topics[ti]), enif_make_copy(env, ref)};
    ERL_NIF_TERM r = call_fn(F_MATCH, env, 3, argv);
    const ERL_NIF_TERM call = ok_value(env, r);
    if (call == r) { /* {error, ebusy | ...}: the caller's own path */
      t->refused++;
      enif_free_env(env);
      enif_free_env(keep);
      continue;
    }
    const ERL_NIF_TERM mycall = enif_make_copy(keep, call);
    enif_free_env(env);
    t->accepted++;
    int cancelled = 0;
    if (rnd(&s) % 100 < t->cancel_pct) {
      usleep(rnd(&s) % 300);
      env = fake_call_env(pid);
      ERL_NIF_TERM cv[2] = {enif_make_copy(env, t->res), enif_make_copy(env, mycall)};
      r = call_fn(F_CANCEL, env, 2, cv);
      if (r == a_true) cancelled = 1;
      else if (r != a_false) violation(t, i, "cancel returned neither true nor false");
      enif_free_env(env);
    }
    if (cancelled) t->cancelled++;
    else take_message(t, i, pid, ti, ref); /* after a cancel that returned false it is there already */
    env = fake_call_env(pid);
    ERL_NIF_TERM cv[2] = {enif_make_copy(env, t->res), enif_make_copy(env, mycall)};
    if (call_fn(F_CANCEL, env, 2, cv) != a_false) violation(t, i, "a second cancel did not return false");
    enif_free_env(env);
    enif_free_env(keep);
  }
  return NULL;
}

static void* writer_run(void* arg) {
  const ERL_NIF_TERM res = *(const ERL_NIF_TERM*)arg;
  const ERL_NIF_TERM a_sub = enif_make_atom(NULL, "sub");
  unsigned long n = 0;
  while (!__atomic_load_n(&g_stop_writer, __ATOMIC_ACQUIRE)) {
    ErlNifEnv* env = fake_call_env(999);
    ERL_NIF_TERM av[2] = {enif_make_copy(env, res), a_sub};
    const ERL_NIF_TERM h = ok_value(env, call_fn(F_ALLOC, env, 2, av));
    unsigned hv;
    if (!enif_get_uint(env, h, &hv)) FAIL("load: alloc_handle failed");
    ERL_NIF_TERM pair = enif_make_tuple2(env, h, enif_make_tuple2(env, a_sub, enif_make_uint64(env, n++)));
    ERL_NIF_TERM rv[3] = {av[0], a_sub, enif_make_list(env, 1, pair)};
    if (call_fn(F_REGISTER, env, 3, rv) != enif_make_atom(NULL, "ok")) FAIL("load: register failed");
    ERL_NIF_TERM lv[3] = {av[0], a_sub, h};
    if (call_fn(F_RELEASE, env, 3, lv) != enif_make_atom(NULL, "ok")) FAIL("load: release_handle failed");
    enif_free_env(env);
    usleep(50);
  }
  return NULL;
}

static void do_load(char* rest) {
  char* resname = next_word(&rest);
  const unsigned threads = (unsigned)atoi(next_word(&rest));
  const unsigned calls = (unsigned)atoi(next_word(&rest));
  const unsigned pct = (unsigned)atoi(next_word(&rest));
  const unsigned seed = (unsigned)atoi(next_word(&rest));
  var* rv = find_var(resname, strlen(resname));
  if (!rv || threads == 0 || threads > 1024) FAIL("load: bad resource name or thread count");
  F_MATCH = find_fn("match_async", 3);
  F_CANCEL = find_fn("cancel", 2);
  F_ALLOC = find_fn("alloc_handle", 2);
  F_REGISTER = find_fn("register", 3);
  F_RELEASE = find_fn("release_handle", 3);
  if (F_MATCH < 0 || F_CANCEL < 0 || F_ALLOC < 0 || F_REGISTER < 0 || F_RELEASE < 0) FAIL("load: table entries missing");
  ErlNifEnv* env = enif_alloc_env();
  const char* p = rest;
  ERL_NIF_TERM l = parse(env, &p), h;
  unsigned nt = 0;
  if (!enif_get_list_length(env, l, &nt) || nt == 0) FAIL("load: a list of topics expected");
  ERL_NIF_TERM* topics = malloc(sizeof *topics * nt);
  for (unsigned i = 0; enif_get_list_cell(env, l, &h, &l); ++i) topics[i] = h;
  ERL_NIF_TERM res = enif_make_copy(env, rv->t);
  load_thread* lt = calloc(threads, sizeof *lt);
  pthread_t* th = malloc(sizeof *th * threads);
  pthread_t wr;
  g_stop_writer = 0;
  fflush(stdout);
  pthread_create(&wr, NULL, writer_run, &res);
  for (unsigned k = 0; k < threads; ++k) {
    lt[k] = (load_thread){k, calls, pct, seed, nt, res, topics, 0, 0, 0, 0, 0};
    pthread_create(&th[k], NULL, load_run, &lt[k]);
  }
  unsigned long acc = 0, ans = 0, can = 0, ref = 0, vio = 0;
  for (unsigned k = 0; k < threads; ++k) {
    pthread_join(th[k], NULL);
    acc += lt[k].accepted;
    ans += lt[k].answered;
    can += lt[k].cancelled;
    ref += lt[k].refused;
    vio += lt[k].violations;
  }
  __atomic_store_n(&g_stop_writer, 1, __ATOMIC_RELEASE);
  pthread_join(wr, NULL);
  long live_calls = -1;
  for (int i = 0; i < fake_resource_types(); ++i) {
    const char* name;
    const long n = fake_live_resources(i, &name);
    if (!strcmp(name, "emqx_trie_gpu_call")) live_calls = n;
  }
  printf("LOAD accepted %lu answered %lu cancelled %lu refused %lu violations %lu live_calls %ld\n", acc, ans, can,
         ref, vio, live_calls);
  free(th);
  free(lt);
  free(topics);
  enif_free_env(env);
}

int main(void) {
  setvbuf(stdout, NULL, _IOLBF, 0);
  g_entry = nif_init();
  g_calls = calloc((size_t)g_entry->num_of_funcs, sizeof *g_calls);
  ErlNifEnv* lenv = enif_alloc_env();
  void* priv = NULL;
  const int lrc = g_entry->load(lenv, &priv, FAKE_NIL);
  enif_free_env(lenv);
  if (lrc) FAIL("load returned %d", lrc);
  char* line = NULL;
  size_t cap = 0;
  ssize_t n;
  while ((n = getline(&line, &cap, stdin)) > 0) {
    while (n > 0 && (line[n - 1] == '\n' || line[n - 1] == '\r')) line[--n] = 0;
    char* rest = line;
    char* cmd = next_word(&rest);
    if (!*cmd || *cmd == '%') continue;
    if (!strcmp(cmd, "call")) do_call(rest);
    else if (!strcmp(cmd, "recv")) do_recv(rest);
    else if (!strcmp(cmd, "ref")) {
      ErlNifEnv* env = enif_alloc_env();
      const ERL_NIF_TERM r = fake_make_ref(env);
      bind_var(next_word(&rest), r);
      fputs("= ", stdout);
      fake_print(stdout, r);
      fputc('\n', stdout);
      enif_free_env(env);
    } else if (!strcmp(cmd, "drop")) drop_var(next_word(&rest));
    else if (!strcmp(cmd, "sleep")) usleep(1000u * (unsigned)atoi(next_word(&rest)));
    else if (!strcmp(cmd, "rc") || !strcmp(cmd, "rc_create")) {
      int* v = cmd[2] ? &g_stub_create_rc : &g_stub_rc;
      if (!v) FAIL("%s: this build has no stubs", cmd);
      *v = atoi(next_word(&rest));
    } else if (!strcmp(cmd, "balance")) print_balance(g_nvars);
    else if (!strcmp(cmd, "load")) do_load(rest);
    else FAIL("unknown line: %s", cmd);
    fflush(stdout);
  }
  free(line);
  while (g_nvars) drop_var(g_vars[g_nvars - 1].name);
  const long left = drain_mailboxes();
  for (int i = 0; i < g_entry->num_of_funcs; ++i)
    printf("T %s/%u %lu\n", g_entry->funcs[i].name, g_entry->funcs[i].arity, g_calls[i]);
  printf("B mailbox %ld\n", left);
  const int bad = print_balance(0);
  free(g_calls);
  fflush(stdout);
  return bad ? 3 : 0;
}
