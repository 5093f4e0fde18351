// Stand-alone: reads a shipsim_config (the bytes of the Python binding's Config) from the file argv[1], runs
// shipsim_create's validate on it and builds its constant block (ast_sac_amd/csrc/shipsim_config_host.hpp). Prints
// "ok <use_grid> <gnx> <gny>" and the grid cells' classes (0 OUT, 1 IN, 2 MIXED) as one line of digits, or validate's
// message and exit status 1. Built and run by tests/test_map_query_cpu.py.
#include <stdio.h>
#include <stdlib.h>

#include "shipsim_config_host.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  shipsim_config cfg;
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(&cfg, sizeof(cfg), 1, f) != 1 || fgetc(f) != EOF) return 2;
  fclose(f);
  char err[256] = "";
  if (config_host::validate(&cfg, err, sizeof(err)) != 0) {
    printf("%s\n", err);
    return 1;
  }
  shipsim::ShipConst sc[SHIPSIM_MAX_SHIPS] = {};
  config_host::ConstBlock cb;
  if (!config_host::const_block(&cfg, sc, cb)) return 2;
  printf("ok %d %d %d\n", (int)cb.use_grid, cb.gnx, cb.gny);
  const size_t cells = (size_t)cb.gnx * cb.gny;
  const unsigned char* flag = (const unsigned char*)(cb.host + cb.grid_off + cells * sizeof(uint64_t));
  for (size_t c = 0; c < cells; ++c) putchar('0' + flag[c]);
  putchar('\n');
  free(cb.host);
  return 0;
}
