/* Test infrastructure only: a small erl_nif runtime, so that c_src/emqx_trie_gpu_nif.c can be
 * linked and run without a BEAM (see fake_erl_nif.h for its rules).  It implements every enif_*
 * the NIF uses with OTP's semantics where the NIF can tell the difference: atoms compare with ==
 * across environments, an environment owns its terms, enif_send copies the message and clears
 * msg_env, resources are reference counted and destructed at zero, enif_alloc is malloc. */
#define _GNU_SOURCE
#include "fake_erl_nif.h"

#include <errno.h>
#include <limits.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#define TAG_ATOM 0x1ul
#define TAG_PID 0x3ul
#define IS_CELL(t) ((t) != 0 && ((t) & 0xFul) == 0)

enum { T_INT, T_UINT, T_DOUBLE, T_BIN, T_TUPLE, T_CONS, T_MAP, T_REF, T_RES };

typedef struct cell {
  struct cell* next;
  int type;
  unsigned n; /* bytes of a binary, arity of a tuple, pairs of a map */
  union {
    long i;
    unsigned long u;
    double d;
    void* res;
  } v;
  ERL_NIF_TERM* e;  /* tuple elements; cons head, tail; map keys then values */
  unsigned char* b; /* binary bytes */
} cell;

struct enif_environment_t {
  cell* cells;
  unsigned self; /* the calling process of a call environment, else 0 */
};

static long g_live_envs;

#define DIE(...)                                  \
  do {                                            \
    fprintf(stderr, "fake_erl_nif: " __VA_ARGS__); \
    fprintf(stderr, "\n");                        \
    abort();                                      \
  } while (0)

/* ---- atoms ---- */
static pthread_mutex_t g_atom_mu = PTHREAD_MUTEX_INITIALIZER;
static char** g_atoms;
static unsigned g_natoms, g_atom_cap;

ERL_NIF_TERM enif_make_atom(ErlNifEnv* env, const char* name) {
  (void)env;
  pthread_mutex_lock(&g_atom_mu);
  unsigned i = 0;
  while (i < g_natoms && strcmp(g_atoms[i], name)) ++i;
  if (i == g_natoms) {
    if (g_natoms == g_atom_cap) {
      g_atom_cap = g_atom_cap ? 2 * g_atom_cap : 64;
      g_atoms = realloc(g_atoms, sizeof(char*) * g_atom_cap);
      if (!g_atoms) DIE("out of memory");
    }
    g_atoms[g_natoms++] = strdup(name);
  }
  pthread_mutex_unlock(&g_atom_mu);
  return ((ERL_NIF_TERM)i << 4) | TAG_ATOM;
}

static int is_atom(ERL_NIF_TERM t) { return (t & 0xFul) == TAG_ATOM; }

static const char* atom_name(ERL_NIF_TERM t) {
  pthread_mutex_lock(&g_atom_mu);
  const unsigned i = (unsigned)(t >> 4);
  const char* s = i < g_natoms ? g_atoms[i] : NULL;
  pthread_mutex_unlock(&g_atom_mu);
  if (!s) DIE("not an atom: %#lx", t);
  return s;
}

int enif_is_atom(ErlNifEnv* env, ERL_NIF_TERM t) {
  (void)env;
  return is_atom(t);
}

int enif_get_atom(ErlNifEnv* env, ERL_NIF_TERM t, char* buf, unsigned cap, ErlNifCharEncoding enc) {
  (void)env;
  (void)enc;
  if (!is_atom(t)) return 0;
  const char* s = atom_name(t);
  const size_t n = strlen(s);
  if (n + 1 > cap) return 0;
  memcpy(buf, s, n + 1);
  return (int)n + 1;
}

/* ---- environments and cells ---- */
ErlNifEnv* enif_alloc_env(void) {
  ErlNifEnv* e = calloc(1, sizeof *e);
  if (e) __atomic_fetch_add(&g_live_envs, 1, __ATOMIC_RELAXED);
  return e;
}

ErlNifEnv* fake_call_env(unsigned pid) {
  ErlNifEnv* e = enif_alloc_env();
  if (!e) DIE("out of memory");
  e->self = pid;
  return e;
}

void enif_clear_env(ErlNifEnv* e) {
  cell* c = e->cells;
  e->cells = NULL;
  while (c) {
    cell* nx = c->next;
    if (c->type == T_RES) enif_release_resource(c->v.res);
    free(c);
    c = nx;
  }
}

void enif_free_env(ErlNifEnv* e) {
  enif_clear_env(e);
  free(e);
  __atomic_fetch_sub(&g_live_envs, 1, __ATOMIC_RELAXED);
}

long fake_live_envs(void) { return __atomic_load_n(&g_live_envs, __ATOMIC_RELAXED); }

static cell* new_cell(ErlNifEnv* env, int type, size_t terms, size_t bytes) {
  if (!env) DIE("a term made without an environment");
  cell* c = malloc(sizeof(cell) + sizeof(ERL_NIF_TERM) * terms + bytes);
  if (!c) DIE("out of memory");
  memset(c, 0, sizeof *c);
  c->type = type;
  c->e = (ERL_NIF_TERM*)(c + 1);
  c->b = (unsigned char*)(c->e + terms);
  c->next = env->cells;
  env->cells = c;
  return c;
}

static cell* as_cell(ERL_NIF_TERM t, int type) {
  if (!IS_CELL(t)) return NULL;
  cell* c = (cell*)t;
  return c->type == type ? c : NULL;
}

/* ---- numbers ---- */
ERL_NIF_TERM enif_make_int64(ErlNifEnv* env, ErlNifSInt64 v) {
  cell* c = new_cell(env, T_INT, 0, 0);
  c->v.i = v;
  return (ERL_NIF_TERM)c;
}
ERL_NIF_TERM enif_make_uint64(ErlNifEnv* env, ErlNifUInt64 v) {
  if (v <= (unsigned long)LONG_MAX) return enif_make_int64(env, (long)v);
  cell* c = new_cell(env, T_UINT, 0, 0);
  c->v.u = v;
  return (ERL_NIF_TERM)c;
}
ERL_NIF_TERM enif_make_int(ErlNifEnv* env, int v) { return enif_make_int64(env, v); }
ERL_NIF_TERM enif_make_uint(ErlNifEnv* env, unsigned v) { return enif_make_int64(env, (long)v); }
ERL_NIF_TERM enif_make_double(ErlNifEnv* env, double d) {
  cell* c = new_cell(env, T_DOUBLE, 0, 0);
  c->v.d = d;
  return (ERL_NIF_TERM)c;
}

int enif_get_int64(ErlNifEnv* env, ERL_NIF_TERM t, ErlNifSInt64* v) {
  (void)env;
  cell* c = as_cell(t, T_INT);
  if (!c) return 0;
  *v = c->v.i;
  return 1;
}
int enif_get_uint64(ErlNifEnv* env, ERL_NIF_TERM t, ErlNifUInt64* v) {
  (void)env;
  cell* c = as_cell(t, T_UINT);
  if (c) {
    *v = c->v.u;
    return 1;
  }
  c = as_cell(t, T_INT);
  if (!c || c->v.i < 0) return 0;
  *v = (unsigned long)c->v.i;
  return 1;
}
int enif_get_int(ErlNifEnv* env, ERL_NIF_TERM t, int* v) {
  long l;
  if (!enif_get_int64(env, t, &l) || l < INT_MIN || l > INT_MAX) return 0;
  *v = (int)l;
  return 1;
}
int enif_get_uint(ErlNifEnv* env, ERL_NIF_TERM t, unsigned* v) {
  long l;
  if (!enif_get_int64(env, t, &l) || l < 0 || l > (long)UINT_MAX) return 0;
  *v = (unsigned)l;
  return 1;
}

/* ---- binaries ---- */
unsigned char* enif_make_new_binary(ErlNifEnv* env, size_t n, ERL_NIF_TERM* out) {
  cell* c = new_cell(env, T_BIN, 0, n);
  c->n = (unsigned)n;
  *out = (ERL_NIF_TERM)c;
  return c->b;
}
ERL_NIF_TERM fake_make_binary(ErlNifEnv* env, const void* p, size_t n) {
  ERL_NIF_TERM t;
  unsigned char* d = enif_make_new_binary(env, n, &t);
  if (n) memcpy(d, p, n);
  return t;
}
int enif_inspect_binary(ErlNifEnv* env, ERL_NIF_TERM t, ErlNifBinary* b) {
  (void)env;
  cell* c = as_cell(t, T_BIN);
  if (!c) return 0;
  b->size = c->n;
  b->data = c->b;
  return 1;
}

/* ---- tuples, lists, maps ---- */
ERL_NIF_TERM enif_make_list_from_array(ErlNifEnv* env, const ERL_NIF_TERM* a, unsigned n) {
  ERL_NIF_TERM l = FAKE_NIL;
  while (n-- > 0) l = enif_make_list_cell(env, a[n], l);
  return l;
}
static ERL_NIF_TERM make_tuple_arr(ErlNifEnv* env, unsigned n, const ERL_NIF_TERM* a) {
  cell* c = new_cell(env, T_TUPLE, n, 0);
  c->n = n;
  for (unsigned i = 0; i < n; ++i) c->e[i] = a[i];
  return (ERL_NIF_TERM)c;
}
ERL_NIF_TERM enif_make_tuple(ErlNifEnv* env, unsigned n, ...) {
  ERL_NIF_TERM a[16];
  va_list ap;
  if (n > 16) DIE("enif_make_tuple: arity %u", n);
  va_start(ap, n);
  for (unsigned i = 0; i < n; ++i) a[i] = va_arg(ap, ERL_NIF_TERM);
  va_end(ap);
  return make_tuple_arr(env, n, a);
}
ERL_NIF_TERM fake_make_tuple_arr(ErlNifEnv* env, unsigned n, const ERL_NIF_TERM* a) {
  return make_tuple_arr(env, n, a);
}
ERL_NIF_TERM enif_make_tuple2(ErlNifEnv* env, ERL_NIF_TERM a, ERL_NIF_TERM b) {
  const ERL_NIF_TERM v[2] = {a, b};
  return make_tuple_arr(env, 2, v);
}
ERL_NIF_TERM enif_make_tuple3(ErlNifEnv* env, ERL_NIF_TERM a, ERL_NIF_TERM b, ERL_NIF_TERM c) {
  const ERL_NIF_TERM v[3] = {a, b, c};
  return make_tuple_arr(env, 3, v);
}
ERL_NIF_TERM enif_make_tuple4(ErlNifEnv* env, ERL_NIF_TERM a, ERL_NIF_TERM b, ERL_NIF_TERM c, ERL_NIF_TERM d) {
  const ERL_NIF_TERM v[4] = {a, b, c, d};
  return make_tuple_arr(env, 4, v);
}
int enif_get_tuple(ErlNifEnv* env, ERL_NIF_TERM t, int* arity, const ERL_NIF_TERM** el) {
  (void)env;
  cell* c = as_cell(t, T_TUPLE);
  if (!c) return 0;
  *arity = (int)c->n;
  *el = c->e;
  return 1;
}

ERL_NIF_TERM enif_make_list(ErlNifEnv* env, unsigned n, ...) {
  ERL_NIF_TERM a[16];
  va_list ap;
  if (n > 16) DIE("enif_make_list: %u elements", n);
  va_start(ap, n);
  for (unsigned i = 0; i < n; ++i) a[i] = va_arg(ap, ERL_NIF_TERM);
  va_end(ap);
  return enif_make_list_from_array(env, a, n);
}
ERL_NIF_TERM enif_make_list_cell(ErlNifEnv* env, ERL_NIF_TERM h, ERL_NIF_TERM t) {
  cell* c = new_cell(env, T_CONS, 2, 0);
  c->e[0] = h;
  c->e[1] = t;
  return (ERL_NIF_TERM)c;
}
int enif_get_list_cell(ErlNifEnv* env, ERL_NIF_TERM l, ERL_NIF_TERM* h, ERL_NIF_TERM* t) {
  (void)env;
  cell* c = as_cell(l, T_CONS);
  if (!c) return 0;
  *h = c->e[0];
  *t = c->e[1];
  return 1;
}
int enif_get_list_length(ErlNifEnv* env, ERL_NIF_TERM l, unsigned* n) {
  (void)env;
  unsigned k = 0;
  cell* c;
  while ((c = as_cell(l, T_CONS))) {
    ++k;
    l = c->e[1];
  }
  if (l != FAKE_NIL) return 0; /* improper, or no list */
  *n = k;
  return 1;
}
int enif_is_list(ErlNifEnv* env, ERL_NIF_TERM t) {
  (void)env;
  return t == FAKE_NIL || as_cell(t, T_CONS) != NULL;
}

ERL_NIF_TERM fake_make_map(ErlNifEnv* env, unsigned n, const ERL_NIF_TERM* k, const ERL_NIF_TERM* v) {
  cell* c = new_cell(env, T_MAP, 2 * (size_t)n, 0);
  c->n = n;
  for (unsigned i = 0; i < n; ++i) {
    c->e[i] = k[i];
    c->e[n + i] = v[i];
  }
  return (ERL_NIF_TERM)c;
}
ERL_NIF_TERM enif_make_new_map(ErlNifEnv* env) { return fake_make_map(env, 0, NULL, NULL); }
int enif_get_map_value(ErlNifEnv* env, ERL_NIF_TERM m, ERL_NIF_TERM key, ERL_NIF_TERM* v) {
  (void)env;
  cell* c = as_cell(m, T_MAP);
  if (!c) return 0;
  for (unsigned i = 0; i < c->n; ++i)
    if (fake_term_eq(c->e[i], key)) {
      *v = c->e[c->n + i];
      return 1;
    }
  return 0;
}
int enif_make_map_put(ErlNifEnv* env, ERL_NIF_TERM m, ERL_NIF_TERM key, ERL_NIF_TERM val, ERL_NIF_TERM* out) {
  cell* c = as_cell(m, T_MAP);
  if (!c) return 0;
  unsigned at = 0;
  while (at < c->n && !fake_term_eq(c->e[at], key)) ++at;
  const unsigned n2 = at < c->n ? c->n : c->n + 1;
  cell* d = new_cell(env, T_MAP, 2 * (size_t)n2, 0);
  d->n = n2;
  for (unsigned i = 0; i < c->n; ++i) {
    d->e[i] = c->e[i];
    d->e[n2 + i] = c->e[c->n + i];
  }
  d->e[at] = key;
  d->e[n2 + at] = val;
  *out = (ERL_NIF_TERM)d;
  return 1;
}

/* ---- references and pids ---- */
static unsigned long g_next_ref = 1;
ERL_NIF_TERM fake_make_ref_id(ErlNifEnv* env, unsigned long id) {
  cell* c = new_cell(env, T_REF, 0, 0);
  c->v.u = id;
  return (ERL_NIF_TERM)c;
}
ERL_NIF_TERM fake_make_ref(ErlNifEnv* env) {
  return fake_make_ref_id(env, __atomic_fetch_add(&g_next_ref, 1, __ATOMIC_RELAXED));
}
int enif_is_ref(ErlNifEnv* env, ERL_NIF_TERM t) {
  (void)env;
  return as_cell(t, T_REF) != NULL;
}
ERL_NIF_TERM fake_make_pid(unsigned pid) { return ((ERL_NIF_TERM)pid << 4) | TAG_PID; }
ErlNifPid* enif_self(ErlNifEnv* env, ErlNifPid* pid) {
  if (!env || !env->self) return NULL; /* not a process-bound environment */
  pid->pid = fake_make_pid(env->self);
  return pid;
}

int enif_is_identical(ERL_NIF_TERM a, ERL_NIF_TERM b) { return fake_term_eq(a, b); }

int fake_term_eq(ERL_NIF_TERM a, ERL_NIF_TERM b) {
  if (a == b) return 1;
  if (!IS_CELL(a) || !IS_CELL(b)) return 0;
  const cell *x = (const cell*)a, *y = (const cell*)b;
  if (x->type != y->type || x->n != y->n) return 0;
  switch (x->type) {
    case T_INT: return x->v.i == y->v.i;
    case T_UINT:
    case T_REF: return x->v.u == y->v.u;
    case T_DOUBLE: return x->v.d == y->v.d;
    case T_RES: return x->v.res == y->v.res;
    case T_BIN: return x->n == 0 || memcmp(x->b, y->b, x->n) == 0;
    default: {
      const unsigned k = x->type == T_CONS ? 2 : x->type == T_MAP ? 2 * x->n : x->n;
      for (unsigned i = 0; i < k; ++i)
        if (!fake_term_eq(x->e[i], y->e[i])) return 0;
      return 1;
    }
  }
}

ERL_NIF_TERM enif_make_copy(ErlNifEnv* env, ERL_NIF_TERM t) {
  if (!IS_CELL(t)) return t;
  const cell* c = (const cell*)t;
  switch (c->type) {
    case T_INT: return enif_make_int64(env, c->v.i);
    case T_UINT: return enif_make_uint64(env, c->v.u);
    case T_DOUBLE: return enif_make_double(env, c->v.d);
    case T_REF: return fake_make_ref_id(env, c->v.u);
    case T_RES: return enif_make_resource(env, c->v.res);
    case T_BIN: return fake_make_binary(env, c->b, c->n);
    case T_CONS: { /* the spine without recursion: lists here can be long */
      ERL_NIF_TERM first = FAKE_NIL;
      cell* prev = NULL;
      ERL_NIF_TERM l = t;
      const cell* k;
      while ((k = as_cell(l, T_CONS))) {
        cell* d = new_cell(env, T_CONS, 2, 0);
        d->e[0] = enif_make_copy(env, k->e[0]);
        d->e[1] = FAKE_NIL;
        if (prev) prev->e[1] = (ERL_NIF_TERM)d;
        else first = (ERL_NIF_TERM)d;
        prev = d;
        l = k->e[1];
      }
      prev->e[1] = enif_make_copy(env, l);
      return first;
    }
    default: {
      const unsigned k = c->type == T_MAP ? 2 * c->n : c->n;
      cell* d = new_cell(env, c->type, k, 0);
      d->n = c->n;
      for (unsigned i = 0; i < k; ++i) d->e[i] = enif_make_copy(env, c->e[i]);
      return (ERL_NIF_TERM)d;
    }
  }
}

ERL_NIF_TERM enif_make_badarg(ErlNifEnv* env) {
  (void)env;
  return FAKE_BADARG;
}

/* ---- allocation ---- */
void* enif_alloc(size_t n) { return malloc(n); }
void* enif_realloc(void* p, size_t n) { return realloc(p, n); }
void enif_free(void* p) { free(p); }

/* ---- resources ---- */
#define RES_LIVE 0x5245534Cul
#define RES_DEAD 0x44454144ul
struct enif_resource_type_t {
  char* name;
  ErlNifResourceDtor* dtor;
  long live;
};
typedef struct {
  unsigned long magic;
  ErlNifResourceType* type;
  long refc;
  unsigned long serial;
} res_hdr; /* 32 bytes: the object behind it stays 16-aligned */

static ErlNifResourceType* g_types[16];
static int g_ntypes;
static unsigned long g_res_serial = 1;

ErlNifResourceType* enif_open_resource_type(ErlNifEnv* env, const char* mod, const char* name,
                                            ErlNifResourceDtor* dtor, ErlNifResourceFlags flags,
                                            ErlNifResourceFlags* tried) {
  (void)env;
  (void)mod;
  (void)flags;
  if (g_ntypes == 16) return NULL;
  ErlNifResourceType* t = calloc(1, sizeof *t);
  if (!t) return NULL;
  t->name = strdup(name);
  t->dtor = dtor;
  g_types[g_ntypes++] = t;
  if (tried) *tried = ERL_NIF_RT_CREATE;
  return t;
}
int fake_resource_types(void) { return g_ntypes; }
long fake_live_resources(int i, const char** name) {
  *name = g_types[i]->name;
  return __atomic_load_n(&g_types[i]->live, __ATOMIC_RELAXED);
}

static res_hdr* hdr_of(void* obj, const char* what) {
  res_hdr* h = (res_hdr*)obj - 1;
  if (h->magic != RES_LIVE) DIE("%s of a resource that is not live (released below zero?)", what);
  return h;
}

void* enif_alloc_resource(ErlNifResourceType* type, size_t size) {
  res_hdr* h = malloc(sizeof *h + size);
  if (!h) return NULL;
  h->magic = RES_LIVE;
  h->type = type;
  h->refc = 1;
  h->serial = __atomic_fetch_add(&g_res_serial, 1, __ATOMIC_RELAXED);
  __atomic_fetch_add(&type->live, 1, __ATOMIC_RELAXED);
  return h + 1;
}
int enif_keep_resource(void* obj) {
  res_hdr* h = hdr_of(obj, "keep");
  __atomic_fetch_add(&h->refc, 1, __ATOMIC_RELAXED);
  return 1;
}
void enif_release_resource(void* obj) {
  res_hdr* h = hdr_of(obj, "release");
  const long left = __atomic_sub_fetch(&h->refc, 1, __ATOMIC_ACQ_REL);
  if (left < 0) DIE("resource %s released below zero", h->type->name);
  if (left > 0) return;
  if (h->type->dtor) h->type->dtor(NULL, obj);
  h->magic = RES_DEAD;
  __atomic_fetch_sub(&h->type->live, 1, __ATOMIC_RELAXED);
  free(h);
}
ERL_NIF_TERM enif_make_resource(ErlNifEnv* env, void* obj) {
  enif_keep_resource(obj);
  cell* c = new_cell(env, T_RES, 0, 0);
  c->v.res = obj;
  return (ERL_NIF_TERM)c;
}
int enif_get_resource(ErlNifEnv* env, ERL_NIF_TERM t, ErlNifResourceType* type, void** obj) {
  (void)env;
  cell* c = as_cell(t, T_RES);
  if (!c || hdr_of(c->v.res, "get")->type != type) return 0;
  *obj = c->v.res;
  return 1;
}

/* ---- mailboxes ---- */
typedef struct msg {
  struct msg* next;
  ErlNifEnv* env;
  ERL_NIF_TERM t;
} msg;
typedef struct {
  pthread_mutex_t mu;
  pthread_cond_t cv;
  msg *head, *tail;
} mailbox;
static mailbox g_box[FAKE_MAX_PIDS];
static pthread_once_t g_box_once = PTHREAD_ONCE_INIT;

static void box_init(void) {
  for (int i = 0; i < FAKE_MAX_PIDS; ++i) {
    pthread_mutex_init(&g_box[i].mu, NULL);
    pthread_condattr_t a;
    pthread_condattr_init(&a);
    pthread_condattr_setclock(&a, CLOCK_MONOTONIC);
    pthread_cond_init(&g_box[i].cv, &a);
    pthread_condattr_destroy(&a);
  }
}

int enif_send(ErlNifEnv* caller, const ErlNifPid* to, ErlNifEnv* msg_env, ERL_NIF_TERM t) {
  (void)caller;
  pthread_once(&g_box_once, box_init);
  const unsigned long id = to->pid >> 4;
  if ((to->pid & 0xFul) != TAG_PID || id == 0 || id >= FAKE_MAX_PIDS) return 0;
  msg* m = malloc(sizeof *m);
  if (!m) DIE("out of memory");
  m->next = NULL;
  m->env = enif_alloc_env();
  if (!m->env) DIE("out of memory");
  m->t = enif_make_copy(m->env, t);
  if (msg_env) enif_clear_env(msg_env); /* as OTP: msg_env is cleared by a successful send */
  mailbox* b = &g_box[id];
  pthread_mutex_lock(&b->mu);
  if (b->tail) b->tail->next = m;
  else b->head = m;
  b->tail = m;
  pthread_cond_signal(&b->cv);
  pthread_mutex_unlock(&b->mu);
  return 1;
}

int fake_recv(unsigned pid, int timeout_ms, ErlNifEnv** env, ERL_NIF_TERM* t) {
  pthread_once(&g_box_once, box_init);
  if (pid == 0 || pid >= FAKE_MAX_PIDS) return 0;
  mailbox* b = &g_box[pid];
  struct timespec until;
  clock_gettime(CLOCK_MONOTONIC, &until);
  until.tv_sec += timeout_ms / 1000;
  until.tv_nsec += (long)(timeout_ms % 1000) * 1000000L;
  if (until.tv_nsec >= 1000000000L) {
    until.tv_nsec -= 1000000000L;
    until.tv_sec += 1;
  }
  pthread_mutex_lock(&b->mu);
  while (!b->head)
    if (pthread_cond_timedwait(&b->cv, &b->mu, &until) == ETIMEDOUT) break;
  msg* m = b->head;
  if (m) {
    b->head = m->next;
    if (!b->head) b->tail = NULL;
  }
  pthread_mutex_unlock(&b->mu);
  if (!m) return 0;
  *env = m->env;
  *t = m->t;
  free(m);
  return 1;
}

/* ---- locks and threads: pthreads ---- */
struct ErlNifRWLock {
  pthread_rwlock_t l;
};
struct ErlNifMutex {
  pthread_mutex_t m;
};
ErlNifRWLock* enif_rwlock_create(char* name) {
  (void)name;
  ErlNifRWLock* l = malloc(sizeof *l);
  if (l) pthread_rwlock_init(&l->l, NULL);
  return l;
}
void enif_rwlock_destroy(ErlNifRWLock* l) {
  pthread_rwlock_destroy(&l->l);
  free(l);
}
void enif_rwlock_rlock(ErlNifRWLock* l) { pthread_rwlock_rdlock(&l->l); }
void enif_rwlock_runlock(ErlNifRWLock* l) { pthread_rwlock_unlock(&l->l); }
void enif_rwlock_rwlock(ErlNifRWLock* l) { pthread_rwlock_wrlock(&l->l); }
void enif_rwlock_rwunlock(ErlNifRWLock* l) { pthread_rwlock_unlock(&l->l); }
ErlNifMutex* enif_mutex_create(char* name) {
  (void)name;
  ErlNifMutex* m = malloc(sizeof *m);
  if (m) pthread_mutex_init(&m->m, NULL);
  return m;
}
void enif_mutex_destroy(ErlNifMutex* m) {
  pthread_mutex_destroy(&m->m);
  free(m);
}
void enif_mutex_lock(ErlNifMutex* m) { pthread_mutex_lock(&m->m); }
void enif_mutex_unlock(ErlNifMutex* m) { pthread_mutex_unlock(&m->m); }
int enif_thread_create(char* name, ErlNifTid* tid, void* (*fn)(void*), void* arg, ErlNifThreadOpts* opts) {
  (void)name;
  (void)opts;
  pthread_t t;
  const int rc = pthread_create(&t, NULL, fn, arg);
  if (!rc) *tid = (ErlNifTid)t;
  return rc;
}
int enif_thread_join(ErlNifTid tid, void** res) { return pthread_join((pthread_t)tid, res); }

/* ---- the term text format (tests/nif_terms.py reads and writes the same) ---- */
static int plain_atom(const char* s) {
  if (!(*s >= 'a' && *s <= 'z')) return 0;
  for (; *s; ++s)
    if (!((*s >= 'a' && *s <= 'z') || (*s >= 'A' && *s <= 'Z') || (*s >= '0' && *s <= '9') || *s == '_' || *s == '@'))
      return 0;
  return 1;
}

void fake_print(FILE* f, ERL_NIF_TERM t) {
  if (t == FAKE_NIL) {
    fputs("[]", f);
  } else if (t == FAKE_BADARG) {
    fputs("badarg", f);
  } else if (is_atom(t)) {
    const char* s = atom_name(t);
    if (plain_atom(s)) fputs(s, f);
    else fprintf(f, "'%s'", s);
  } else if ((t & 0xFul) == TAG_PID) {
    fprintf(f, "@%lu", t >> 4);
  } else if (!IS_CELL(t)) {
    fprintf(f, "?%#lx", t);
  } else {
    const cell* c = (const cell*)t;
    switch (c->type) {
      case T_INT: fprintf(f, "%ld", c->v.i); break;
      case T_UINT: fprintf(f, "%lu", c->v.u); break;
      case T_DOUBLE: {
        char buf[64];
        snprintf(buf, sizeof buf, "%.17g", c->v.d);
        fputs(buf, f);
        if (!strpbrk(buf, ".en")) fputs(".0", f); /* a float keeps its point */
        break;
      }
      case T_REF: fprintf(f, "&%lu", c->v.u); break;
      case T_RES: {
        const res_hdr* h = (const res_hdr*)c->v.res - 1;
        fprintf(f, "%%%s:%lu", h->type->name, h->serial);
        break;
      }
      case T_BIN:
        fputs("<<", f);
        for (unsigned i = 0; i < c->n; ++i) fprintf(f, "%02x", c->b[i]);
        fputs(">>", f);
        break;
      case T_TUPLE:
        fputc('{', f);
        for (unsigned i = 0; i < c->n; ++i) {
          if (i) fputc(',', f);
          fake_print(f, c->e[i]);
        }
        fputc('}', f);
        break;
      case T_MAP:
        fputs("#{", f);
        for (unsigned i = 0; i < c->n; ++i) {
          if (i) fputc(',', f);
          fake_print(f, c->e[i]);
          fputs("=>", f);
          fake_print(f, c->e[c->n + i]);
        }
        fputc('}', f);
        break;
      case T_CONS: {
        fputc('[', f);
        ERL_NIF_TERM l = t;
        const cell* k;
        int first = 1;
        while ((k = as_cell(l, T_CONS))) {
          if (!first) fputc(',', f);
          first = 0;
          fake_print(f, k->e[0]);
          l = k->e[1];
        }
        if (l != FAKE_NIL) {
          fputc('|', f);
          fake_print(f, l);
        }
        fputc(']', f);
        break;
      }
      default: fprintf(f, "?cell%d", c->type);
    }
  }
}
